// tracer_kernels.hip -- tracer particles (castro.do_tracer_particles), 3-D Cartesian.  The container is AMReX's
// AmrTracerParticleContainer [3P]; what it does is restated from its published algorithm (DESIGN.md "Tracer particles"):
//   k_tracer_advect<PASS>  AdvectWithUcc: the two passes of the midpoint rule over the particles of one level -- cell-centred
//                          cloud-in-cell gather of u = mom * (1 / rho) from the half-time state of the particle's box, formed at
//                          every stencil corner (the reference's Ucc holds that value in that zone: Source/particles/
//                          CastroParticles.cpp:252-281), no velocity array
//   k_tracer_locate        Redistribute: periodic wrap, invalidation outside a non-periodic domain, finest level with a valid box
//                          over the particle's cell, the ngrow fallback on lev_min, the "lost particle" flag
//   k_tracer_sample        the cloud-in-cell gather of state components at the particle positions (TimestampParticles, :195-247)
//   k_tracer_count         particles per zone (ParticleDerive, :125-133): 32-bit integer atomics -- the sums do not depend on
//                          the arrival order
// and the migration between ranks (k_tracer_dest, k_tracer_scan, k_tracer_pack, k_tracer_unpack, further down).
// One thread per particle over SoA arrays, 256-thread blocks, 64-bit offsets.  These four never change the particle order (only a
// migration does, into new arrays), so the accesses of a wave are a gather by nature: eight corners x four components through L2; whether sorting by box would pay is unmeasured.
//
// Bounds.  Every stencil index is clamped to the array it reads, a particle whose `grid` is no box of the table (or a box of
// another rank: an entry without a FAB) is skipped, and a
// count outside its FAB is dropped: no input makes a kernel touch memory outside a FAB.  Each particle and pass that had to
// clamp (or was skipped) adds 1 to flags[0], each lost particle 1 to flags[1]; the driver turns either into an error.
//
// Numerics.  Cell indices are discrete decisions: this file is compiled with contraction off and signed zeros kept in the
// `contract` build too (Makefile), so both builds produce the bits of the numpy restatement (tests/tracer_ref.py): the
// loop nest kk, jj, ii with val += sx[ii] * sy[jj] * sz[kk] * data left to right, 1.0 / rho by IEEE division.
#include <hip/hip_runtime.h>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../include/castro_hydro_amd.h"
#include "hydro_device.h"
#include "ctu_kernels.h"

namespace cad {

// floor(l) as a zone index; values no int holds (NaN included) become +-10^9, which every clamp and box test rejects
__device__ __forceinline__ int tr_floor(double l)
{
    const double fl = floor(l);
    if (fabs(fl) < 1.0e9) return (int)fl;
    return fl > 0.0 ? 1000000000 : -1000000000;
}

// the 2 x 2 x 2 stencil of a position in one box: clamped offsets into the FAB and the weights
struct TrStencil {
    long ox[2], oy[2], oz[2];
    double sx[2], sy[2], sz[2];
    int clamped;
};

__device__ __forceinline__ void tr_stencil_dir(double pos, double plo, double dxi, int alo, int ahi, long stride, long o[2],
                                               double s[2], int& clamped)
{
    const double l = (pos - plo) * dxi - 0.5;
    const int i = tr_floor(l);
    const double f = l - (double)i;
    s[0] = 1.0 - f;
    s[1] = f;
    for (int q = 0; q < 2; ++q) {
        long c = (long)i + q;
        if (c < alo) { c = alo; clamped = 1; }
        if (c > ahi) { c = ahi; clamped = 1; }
        o[q] = stride * (c - alo);
    }
}

__device__ __forceinline__ TrStencil tr_stencil(const TrBoxDev& B, const TrGeom& G, const double* dxi, double x, double y, double z)
{
    TrStencil S;
    S.clamped = 0;
    tr_stencil_dir(x, G.plo[0], dxi[0], B.alo[0], B.ahi[0], 1, S.ox, S.sx, S.clamped);
    tr_stencil_dir(y, G.plo[1], dxi[1], B.alo[1], B.ahi[1], B.F.sy, S.oy, S.sy, S.clamped);
    tr_stencil_dir(z, G.plo[2], dxi[2], B.alo[2], B.ahi[2], B.F.sz, S.oz, S.sz, S.clamped);
    return S;
}

// the one gather: component `comp` of the FAB, or (VEL) that component times 1 / rho, at the eight corners
template <bool VEL>
__device__ __forceinline__ double tr_gather(const TrBoxDev& B, const TrStencil& S, int comp)
{
    const double* __restrict__ p = B.F.p;
    double val = 0.0;
    for (int kk = 0; kk < 2; ++kk)
        for (int jj = 0; jj < 2; ++jj)
            for (int ii = 0; ii < 2; ++ii) {
                const long c = S.ox[ii] + S.oy[jj] + S.oz[kk];
                double d = p[c + B.F.sn * comp];
                if (VEL) d = d * (1.0 / p[c + B.F.sn * URHO]);
                val += S.sx[ii] * S.sy[jj] * S.sz[kk] * d;
            }
    return val;
}

// the particle is one this launch acts on; its box into b.  A `grid` outside the table, or one that names an entry without a FAB
// (a box of another rank), counts as a clamp and skips the particle
__device__ __forceinline__ bool tr_mine(const TrBoxDev* __restrict__ tab, const castro_amd_tracers& T, long t, int level, int nbox,
                                        int* __restrict__ flags, int& b)
{
    if (T.id[t] <= 0 || T.level[t] != level) return false;
    b = T.grid[t];
    if (b < 0 || b >= nbox || tab[b].F.p == nullptr) { atomicAdd(&flags[0], 1); return false; }
    return true;
}

template <int PASS>
__global__ void __launch_bounds__(256) k_tracer_advect(const TrBoxDev* __restrict__ tab, int nbox, int level, TrGeom G, double dt,
                                                       castro_amd_tracers T, int* __restrict__ flags)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T.n) return;
    int b;
    if (!tr_mine(tab, T, t, level, nbox, flags, b)) return;
    const TrBoxDev B = tab[b];
    const double x = T.x[t], y = T.y[t], z = T.z[t];
    const TrStencil S = tr_stencil(B, G, G.dxi[0], x, y, z);
    if (S.clamped) atomicAdd(&flags[0], 1);
    const double vx = tr_gather<true>(B, S, UMX), vy = tr_gather<true>(B, S, UMY), vz = tr_gather<true>(B, S, UMZ);
    if (PASS == 0) {
        T.r0[t] = x; T.r1[t] = y; T.r2[t] = z;
        T.x[t] = x + 0.5 * dt * vx;
        T.y[t] = y + 0.5 * dt * vy;
        T.z[t] = z + 0.5 * dt * vz;
    } else {
        T.x[t] = T.r0[t] + dt * vx;
        T.y[t] = T.r1[t] + dt * vy;
        T.z[t] = T.r2[t] + dt * vz;
        T.r0[t] = vx; T.r1[t] = vy; T.r2[t] = vz;
    }
}

__global__ void __launch_bounds__(256) k_tracer_sample(const TrBoxDev* __restrict__ tab, int nbox, int level, TrGeom G, TrComps C,
                                                       castro_amd_tracers T, double* __restrict__ out, int* __restrict__ flags)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T.n) return;
    int b;
    if (!tr_mine(tab, T, t, level, nbox, flags, b)) return;
    const TrBoxDev B = tab[b];
    const TrStencil S = tr_stencil(B, G, G.dxi[0], T.x[t], T.y[t], T.z[t]);
    if (S.clamped) atomicAdd(&flags[0], 1);
    for (int c = 0; c < C.n; ++c) out[(long)c * T.n + t] = tr_gather<false>(B, S, C.comp[c]);
}

__device__ __forceinline__ int tr_find_box(const TrBoxDev* __restrict__ tab, int b0, int b1, int grow, int i, int j, int k)
{
    for (int b = b0; b < b1; ++b) {
        const TrBoxDev& B = tab[b];
        if (i >= B.vlo[0] - grow && i <= B.vhi[0] + grow && j >= B.vlo[1] - grow && j <= B.vhi[1] + grow
            && k >= B.vlo[2] - grow && k <= B.vhi[2] + grow) return b - b0;
    }
    return -1;
}

// tab: the boxes of level l are tab[G.start[l], G.start[l + 1])
__global__ void __launch_bounds__(256) k_tracer_locate(const TrBoxDev* __restrict__ tab, TrGeom G, int lev_min, int lev_max, int ngrow,
                                                       castro_amd_tracers T, int* __restrict__ flags)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T.n) return;
    const int id = T.id[t];
    if (id <= 0 || T.level[t] < lev_min) return;
    double pos[3] = {T.x[t], T.y[t], T.z[t]};
    bool outside = false;
    for (int d = 0; d < 3; ++d) {
        const double plo = G.plo[d], phi = G.phi[d];
        if (G.periodic[d]) {
            // a position many domain lengths away (or not finite) is not walked back: it ends as a lost particle
            if (fabs(pos[d] - plo) < 1.0e3 * (phi - plo)) {
                while (pos[d] >= phi) pos[d] -= (phi - plo);
                while (pos[d] < plo) pos[d] += (phi - plo);
                if (pos[d] == phi) pos[d] = plo;
            }
        } else if (!(pos[d] >= plo && pos[d] < phi)) {
            outside = true;
        }
    }
    T.x[t] = pos[0]; T.y[t] = pos[1]; T.z[t] = pos[2];
    if (outside) { T.id[t] = -id; return; }
    for (int l = lev_max; l >= lev_min; --l) {
        const int i = tr_floor((pos[0] - G.plo[0]) * G.dxi[l][0]), j = tr_floor((pos[1] - G.plo[1]) * G.dxi[l][1]),
                  k = tr_floor((pos[2] - G.plo[2]) * G.dxi[l][2]);
        int b = tr_find_box(tab, G.start[l], G.start[l + 1], 0, i, j, k);
        if (b < 0 && l == lev_min && ngrow > 0) b = tr_find_box(tab, G.start[l], G.start[l + 1], ngrow, i, j, k);
        if (b >= 0) { T.level[t] = l; T.grid[t] = b; return; }
    }
    atomicAdd(&flags[1], 1);
}

// tab[b].F.p addresses the int32 zones of count FAB b (one component)
__global__ void __launch_bounds__(256) k_tracer_count(const TrBoxDev* __restrict__ tab, int nbox, int level, TrGeom G,
                                                      castro_amd_tracers T)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T.n) return;
    if (T.id[t] <= 0 || T.level[t] != level) return;
    const int b = T.grid[t];
    if (b < 0 || b >= nbox) return;
    const TrBoxDev& B = tab[b];
    if (B.F.p == nullptr) return;               // a box of another rank: no FAB here
    const int i = tr_floor((T.x[t] - G.plo[0]) * G.dxi[0][0]), j = tr_floor((T.y[t] - G.plo[1]) * G.dxi[0][1]),
              k = tr_floor((T.z[t] - G.plo[2]) * G.dxi[0][2]);
    if (i < B.alo[0] || i > B.ahi[0] || j < B.alo[1] || j > B.ahi[1] || k < B.alo[2] || k > B.ahi[2]) return;
    int* p = reinterpret_cast<int*>(B.F.p);
    atomicAdd(&p[(long)(i - B.alo[0]) + B.F.sy * (long)(j - B.alo[1]) + B.F.sz * (long)(k - B.alo[2])], 1);
}

static inline bool tr_grid(long n, unsigned& blocks)
{
    const long nb = (n + 255) / 256;
    if (nb >= 0x7fffffffL) return false;
    blocks = (unsigned)nb;
    return true;
}

// The tables are kept on the device per content (TableCache, dev_table.h): fully initialised bytes
int launch_tracer_advect(int nbox, const TrBoxDev* boxes, int level, const TrGeom& G, double dt, int ipass, const castro_amd_tracers& T,
                         int* d_flags, TableCache* tables, hipStream_t stream, Profiler* prof)
{
    unsigned blocks;
    if (T.n == 0 || nbox == 0) return 0;
    if (!tr_grid(T.n, blocks)) return CASTRO_AMD_ERR_ARG;
    const TrBoxDev* dtab = nullptr;
    const int rt = tables->find(boxes, (size_t)nbox, stream, dtab);
    if (rt != 0) return rt;
    prof_begin(prof, ipass == 0 ? "k_tracer_advect<0>" : "k_tracer_advect<1>", stream);
    if (ipass == 0) hipLaunchKernelGGL(k_tracer_advect<0>, dim3(blocks), dim3(256), 0, stream, dtab, nbox, level, G, dt, T, d_flags);
    else hipLaunchKernelGGL(k_tracer_advect<1>, dim3(blocks), dim3(256), 0, stream, dtab, nbox, level, G, dt, T, d_flags);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

int launch_tracer_sample(int nbox, const TrBoxDev* boxes, int level, const TrGeom& G, const TrComps& C, const castro_amd_tracers& T,
                         double* d_out, int* d_flags, TableCache* tables, hipStream_t stream, Profiler* prof)
{
    unsigned blocks;
    if (T.n == 0 || nbox == 0) return 0;
    if (!tr_grid(T.n, blocks)) return CASTRO_AMD_ERR_ARG;
    const TrBoxDev* dtab = nullptr;
    const int rt = tables->find(boxes, (size_t)nbox, stream, dtab);
    if (rt != 0) return rt;
    prof_begin(prof, "k_tracer_sample", stream);
    hipLaunchKernelGGL(k_tracer_sample, dim3(blocks), dim3(256), 0, stream, dtab, nbox, level, G, C, T, d_out, d_flags);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

int launch_tracer_locate(int nbox, const TrBoxDev* boxes, const TrGeom& G, int lev_min, int lev_max, int ngrow,
                         const castro_amd_tracers& T, int* d_flags, TableCache* tables, hipStream_t stream, Profiler* prof)
{
    unsigned blocks;
    if (T.n == 0) return 0;
    if (!tr_grid(T.n, blocks)) return CASTRO_AMD_ERR_ARG;
    const TrBoxDev* dtab = nullptr;
    if (nbox > 0) {
        const int rt = tables->find(boxes, (size_t)nbox, stream, dtab);
        if (rt != 0) return rt;
    }
    prof_begin(prof, "k_tracer_locate", stream);
    hipLaunchKernelGGL(k_tracer_locate, dim3(blocks), dim3(256), 0, stream, dtab, G, lev_min, lev_max, ngrow, T, d_flags);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

int launch_tracer_count(int nbox, const TrBoxDev* boxes, int level, const TrGeom& G, const castro_amd_tracers& T, TableCache* tables,
                        hipStream_t stream, Profiler* prof)
{
    unsigned blocks;
    if (T.n == 0 || nbox == 0) return 0;
    if (!tr_grid(T.n, blocks)) return CASTRO_AMD_ERR_ARG;
    const TrBoxDev* dtab = nullptr;
    const int rt = tables->find(boxes, (size_t)nbox, stream, dtab);
    if (rt != 0) return rt;
    prof_begin(prof, "k_tracer_count", stream);
    hipLaunchKernelGGL(k_tracer_count, dim3(blocks), dim3(256), 0, stream, dtab, nbox, level, G, T);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

// ---- migration between ranks ------------------------------------------------------------------------------------------------------
// A stable partition of the particle arrays by destination rank in three launches, none of which waits on another workgroup:
//   k_tracer_dest   dest[t] and the counts of every block per destination, hist[block][rank] (LDS integer atomics: sums)
//   k_tracer_scan   one workgroup per rank: the exclusive prefix of its column of hist over the blocks, in place, and the total
//                   (to counts[rank] and to the row behind the last block, where the pack reads it)
//   k_tracer_pack   the rank of a particle among those of its block with the same destination -- the waves peel the keys they
//                   hold with ballots (most particles stay: very few keys per wave), per-wave totals in LDS -- then the copy:
//                   stayers to the `out` arrays, leavers to 64-byte wire records, contiguous per destination in rank order
// The order is the input order within every destination; integer work and bit copies only.
// Wire record (eight 8-byte slots): the bits of x y z r0 r1 r2, then id | cpu << 32, then level | grid << 32 (unsigned halves).

__global__ void __launch_bounds__(256) k_tracer_dest(const int* __restrict__ owners, TrOwners O, int nranks, int myrank,
                                                     castro_amd_tracers T, int* __restrict__ dest, int* __restrict__ hist)
{
    __shared__ int s_cnt[CAD_TRACER_MAX_RANKS];
    for (int r = threadIdx.x; r < nranks; r += 256) s_cnt[r] = 0;
    __syncthreads();
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < T.n) {
        int d = myrank;
        const int l = T.level[t], g = T.grid[t];
        if (T.id[t] > 0 && l >= 0 && l < O.nlev && g >= 0 && g < O.start[l + 1] - O.start[l]) d = owners[O.start[l] + g];
        dest[t] = d;
        atomicAdd(&s_cnt[d], 1);
    }
    __syncthreads();
    for (int r = threadIdx.x; r < nranks; r += 256) hist[(long)blockIdx.x * nranks + r] = s_cnt[r];
}

// inclusive sum over the 256 threads of a block through s (every thread calls it)
__device__ __forceinline__ int tr_block_scan(int* s, int tid, int v)
{
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    return s[tid];
}

__global__ void __launch_bounds__(256) k_tracer_scan(int* __restrict__ hist, long nblocks, int nranks, int* __restrict__ counts)
{
    __shared__ int s[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    int carry = 0;
    for (long base = 0; base < nblocks; base += 256) {          // the same trip count in every thread
        const long b = base + tid;
        const int v = b < nblocks ? hist[b * nranks + r] : 0;
        const int incl = tr_block_scan(s, tid, v);
        if (b < nblocks) hist[b * nranks + r] = carry + incl - v;
        carry += s[255];
        __syncthreads();
    }
    if (tid == 0) { counts[r] = carry; hist[nblocks * nranks + r] = carry; }
}

__device__ __forceinline__ unsigned long long tr_pair(int lo, int hi)
{
    return (unsigned long long)(unsigned)lo | ((unsigned long long)(unsigned)hi << 32);
}

__global__ void __launch_bounds__(256) k_tracer_pack(const int* __restrict__ hist, long nblocks, int nranks, int myrank,
                                                     castro_amd_tracers T, const int* __restrict__ dest, castro_amd_tracers out,
                                                     long long* __restrict__ wire, long nwire)
{
    __shared__ int s_wave[4][CAD_TRACER_MAX_RANKS];             // per wave and key: the count, then the offset of the wave's first
    __shared__ int s_scan[256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int r = tid; r < 4 * CAD_TRACER_MAX_RANKS; r += 256) (&s_wave[0][0])[r] = 0;
    // first record of every destination in the wire buffer: the leavers to lower ranks come first (thread r: rank r)
    const int tot = (tid < nranks && tid != myrank) ? hist[nblocks * nranks + tid] : 0;
    const int wirebase = tr_block_scan(s_scan, tid, tot) - tot;

    const long t = (long)blockIdx.x * blockDim.x + tid;
    int key = t < T.n ? dest[t] : -1;
    if (key >= nranks) key = -1;                                // not a value k_tracer_dest writes: nothing is indexed with it
    int below = 0;
    unsigned long long todo = __ballot(key >= 0);               // wave-uniform: every lane runs the loop
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader);
        const unsigned long long same = __ballot(key == k);
        if (key == k) below = __popcll(same & ((1ull << lane) - 1ull));
        if (lane == leader) s_wave[w][k] = __popcll(same);
        todo &= ~same;
    }
    __syncthreads();
    if (tid < nranks) {
        int acc = (tid == myrank ? 0 : wirebase) + hist[(long)blockIdx.x * nranks + tid];
        for (int q = 0; q < 4; ++q) { const int c = s_wave[q][tid]; s_wave[q][tid] = acc; acc += c; }
    }
    __syncthreads();
    if (key < 0) return;
    const long at = (long)s_wave[w][key] + below;
    const int cpu = T.cpu ? T.cpu[t] : 0;
    if (key == myrank) {
        if (at >= out.n) return;
        out.x[at] = T.x[t]; out.y[at] = T.y[t]; out.z[at] = T.z[t];
        out.r0[at] = T.r0[t]; out.r1[at] = T.r1[t]; out.r2[at] = T.r2[t];
        out.id[at] = T.id[t]; out.level[at] = T.level[t]; out.grid[at] = T.grid[t];
        if (out.cpu) out.cpu[at] = cpu;
    } else {
        if (at >= nwire) return;
        ulonglong2* rec = reinterpret_cast<ulonglong2*>(wire + 8 * at);                 // four 16-byte stores
        rec[0] = make_ulonglong2((unsigned long long)__double_as_longlong(T.x[t]), (unsigned long long)__double_as_longlong(T.y[t]));
        rec[1] = make_ulonglong2((unsigned long long)__double_as_longlong(T.z[t]), (unsigned long long)__double_as_longlong(T.r0[t]));
        rec[2] = make_ulonglong2((unsigned long long)__double_as_longlong(T.r1[t]), (unsigned long long)__double_as_longlong(T.r2[t]));
        rec[3] = make_ulonglong2(tr_pair(T.id[t], cpu), tr_pair(T.level[t], T.grid[t]));
    }
}

__global__ void __launch_bounds__(256) k_tracer_unpack(const long long* __restrict__ wire, long nrecv, castro_amd_tracers out, long at0)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nrecv) return;
    const ulonglong2* rec = reinterpret_cast<const ulonglong2*>(wire + 8 * t);
    const ulonglong2 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
    const long at = at0 + t;
    out.x[at] = __longlong_as_double((long long)a.x); out.y[at] = __longlong_as_double((long long)a.y);
    out.z[at] = __longlong_as_double((long long)b.x); out.r0[at] = __longlong_as_double((long long)b.y);
    out.r1[at] = __longlong_as_double((long long)c.x); out.r2[at] = __longlong_as_double((long long)c.y);
    out.id[at] = (int)(unsigned)(d.x & 0xffffffffull);
    if (out.cpu) out.cpu[at] = (int)(unsigned)(d.x >> 32);
    out.level[at] = (int)(unsigned)(d.y & 0xffffffffull);
    out.grid[at] = (int)(unsigned)(d.y >> 32);
}

// hist[nblocks + 1][nranks] of the context, grown behind the work queued on `stream`
static int tr_migrate_scratch(TrMigrateWorkspace* ws, long nblocks, int nranks, hipStream_t stream)
{
    const size_t need = (size_t)(nblocks + 1) * (size_t)nranks;
    if (need > ws->ints) {
        if (ws->hist) { (void)hipStreamSynchronize(stream); (void)hipFree(ws->hist); }
        ws->hist = nullptr; ws->ints = 0;
        if (hipMalloc((void**)&ws->hist, 2 * need * sizeof(int)) != hipSuccess) { ws->hist = nullptr; return CASTRO_AMD_ERR_NOMEM; }
        ws->ints = 2 * need;
    }
    return 0;
}

int launch_tracer_migrate_count(const int* owners, int nown, const TrOwners& O, int nranks, int myrank, const castro_amd_tracers& T,
                                int* d_dest, int* d_counts, TrMigrateWorkspace* ws, TableCache* tables, hipStream_t stream,
                                Profiler* prof)
{
    ws->n = -1;
    if (T.n == 0) {                                            // no launch: the counts are zero
        if (hipMemsetAsync(d_counts, 0, (size_t)nranks * sizeof(int), stream) != hipSuccess) return CASTRO_AMD_ERR_HIP;
        ws->n = 0; ws->nranks = nranks;
        return 0;
    }
    unsigned blocks;
    if (T.n > 0x7fffffffLL || !tr_grid(T.n, blocks)) return CASTRO_AMD_ERR_ARG;     // the counts are int32
    const int* down = nullptr;
    if (nown > 0) {
        const int rt = tables->find(owners, (size_t)nown, stream, down);
        if (rt != 0) return rt;
    }
    const int rs = tr_migrate_scratch(ws, (long)blocks, nranks, stream);
    if (rs != 0) return rs;
    prof_begin(prof, "k_tracer_dest", stream);
    hipLaunchKernelGGL(k_tracer_dest, dim3(blocks), dim3(256), 0, stream, down, O, nranks, myrank, T, d_dest, ws->hist);
    prof_end(prof, stream);
    prof_begin(prof, "k_tracer_scan", stream);
    hipLaunchKernelGGL(k_tracer_scan, dim3((unsigned)nranks), dim3(256), 0, stream, ws->hist, (long)blocks, nranks, d_counts);
    prof_end(prof, stream);
    if (hipGetLastError() != hipSuccess) return CASTRO_AMD_ERR_HIP;
    ws->n = T.n; ws->nranks = nranks;
    return 0;
}

int launch_tracer_migrate_pack(int nranks, int myrank, const castro_amd_tracers& T, const int* d_dest, const castro_amd_tracers& out,
                               long long* d_wire, long long nwire, TrMigrateWorkspace* ws, hipStream_t stream, Profiler* prof)
{
    if (ws->n != T.n || ws->nranks != nranks) return CASTRO_AMD_ERR_ARG;           // not the particles of the preceding count call
    unsigned blocks;
    if (T.n == 0) return 0;
    if (!tr_grid(T.n, blocks)) return CASTRO_AMD_ERR_ARG;
    prof_begin(prof, "k_tracer_pack", stream);
    hipLaunchKernelGGL(k_tracer_pack, dim3(blocks), dim3(256), 0, stream, ws->hist, (long)blocks, nranks, myrank, T, d_dest, out, d_wire,
                       (long)nwire);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

int launch_tracer_unpack(const long long* d_wire, long long nrecv, const castro_amd_tracers& out, long long at, hipStream_t stream,
                         Profiler* prof)
{
    unsigned blocks;
    if (nrecv == 0) return 0;
    if (!tr_grid(nrecv, blocks)) return CASTRO_AMD_ERR_ARG;
    prof_begin(prof, "k_tracer_unpack", stream);
    hipLaunchKernelGGL(k_tracer_unpack, dim3(blocks), dim3(256), 0, stream, d_wire, (long)nrecv, out, (long)at);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

} // namespace cad

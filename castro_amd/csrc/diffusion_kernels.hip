// diffusion_kernels.hip -- explicit thermal diffusion (castro.diffuse_temp = 1, Source/diffusion/):
//   k_temp_diffusion        source(UEDEN, UEINT) += mult * div(k grad T) for every box of a table in one launch
//                           (Castro::getTempDiffusionTerm + add_temp_diffusion_to_source, Castro_diffusion.cpp:78-176)
//   k_estdt_temp_diffusion  min over the zones of 0.5 dx^2 / D (Castro::estdt_temp_diffusion, timestep.cpp:259-345)
// The operator the reference applies is AMReX's MLABecLaplacian [3P, not in the reference tree]: the 7-point stencil below is a
// restatement (include/castro_hydro_amd.h).  Constant conductivity only (conductivity.const_conductivity).
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/castro_hydro_amd.h"
#include "hydro_device.h"
#include "ctu_kernels.h"

namespace cad {

static inline int diff_launch_status() { return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP; }

__device__ __forceinline__ long didx(const DFab& f, int i, int j, int k)
{
    return (long)(i - f.lo[0]) + f.sy * (long)(j - f.lo[1]) + f.sz * (long)(k - f.lo[2]);
}

// fill_temp_cond (diffusion_util.cpp:12-58) for a constant conductivity: zero at or below the cutoff density, ramped linearly
// up to diffuse_cutoff_density_hi, times diffuse_cond_scale_fac.  The division of the ramp is taken only by the zones inside it.
__device__ __forceinline__ double cond_cc(const DiffDev& D, double rho)
{
    double cond = 0.0;
    if (rho > D.cutoff) {
        cond = D.cond;
        if (rho < D.cutoff_hi) {
            const double multiplier = (rho - D.cutoff) / (D.cutoff_hi - D.cutoff);
            cond = cond * multiplier;
        }
    }
    return D.scale * cond;
}

// one direction of the operator: b(hi face) (T+ - T) - b(lo face) (T - T-), b = the mean of the two cell-centred
// conductivities; a face on a physical domain boundary carries no flux (homogeneous Neumann), whatever its ghost zone holds
__device__ __forceinline__ double diff_flux(double Tm, double T0, double Tp, double km, double k0, double kp, bool phys_lo, bool phys_hi)
{
    const double bhi = 0.5 * (kp + k0);
    const double blo = 0.5 * (k0 + km);
    const double fhi = phys_hi ? 0.0 : bhi * (Tp - T0);
    const double flo = phys_lo ? 0.0 : blo * (T0 - Tm);
    return fhi - flo;
}

// The running state of one (i, j) column of one FAB as the thread marches along k: temperature and conductivity of the zones
// k-1, k, k+1 stay in registers, so every plane of rho and T is fetched once by its own column (plus the four in-plane
// neighbours of the centre plane, which the neighbouring lanes / rows have just pulled into L1 / L2).
struct DiffColumn {
    const double* __restrict__ rho;
    const double* __restrict__ T;
    long c, sy, sz;                 // offset of (i, j, k) in a component plane, row and plane strides
    double Tm, T0, Tp, km, k0, kp;

    __device__ __forceinline__ void start(const DFab& U, const DiffDev& D, int i, int j, int k)
    {
        rho = U.p + U.sn * URHO; T = U.p + U.sn * UTEMP;
        sy = U.sy; sz = U.sz;
        c = didx(U, i, j, k);
        Tm = T[c - sz]; km = cond_cc(D, rho[c - sz]);
        T0 = T[c];      k0 = cond_cc(D, rho[c]);
    }
    __device__ __forceinline__ double term(const DiffDev& D, bool pxl, bool pxh, bool pyl, bool pyh, bool pzl, bool pzh)
    {
        Tp = T[c + sz]; kp = cond_cc(D, rho[c + sz]);
        const double fx = diff_flux(T[c - 1], T0, T[c + 1], cond_cc(D, rho[c - 1]), k0, cond_cc(D, rho[c + 1]), pxl, pxh);
        const double fy = diff_flux(T[c - sy], T0, T[c + sy], cond_cc(D, rho[c - sy]), k0, cond_cc(D, rho[c + sy]), pyl, pyh);
        const double fz = diff_flux(Tm, T0, Tp, km, k0, kp, pzl, pzh);
        return D.dh[0] * fx + D.dh[1] * fy + D.dh[2] * fz;
    }
    __device__ __forceinline__ void advance()
    {
        Tm = T0; T0 = Tp; km = k0; k0 = kp; c += sz;
    }
};

constexpr int DIFF_TJ = 4;        // rows (j) of a workgroup: one wave of 64 consecutive i per row
constexpr int DIFF_KC = 32;       // zones a thread marches along k: the two halo planes of a chunk cost 2 / 32 of its reads

// TWO: the time-centred corrector of construct_new_diff_source, += m1 * DiffTerm(U) then += m2 * DiffTerm(U2), one pass.
// init != 0: the two source components start from 0.0 instead of from what the FAB holds (the `source = 0` of a source stage
// without a fill of its own).  Out.p: the bare DiffTerm(U) into a one-component FAB as well.
template <bool TWO>
__global__ void __launch_bounds__(64 * DIFF_TJ) k_temp_diffusion(const DiffBoxDev* __restrict__ tab, const int* __restrict__ start, int nbox,
                                                                 unsigned nb, DiffDev D, double m1, double m2, int init)
{
    // the workgroups are dealt round robin over the 8 XCDs: renumbered so that an XCD works on consecutive tiles, whose rows are
    // each other's j +- 1 neighbours and share its L2 (the tail that does not fill a round of 8 keeps its place)
    unsigned bid = blockIdx.x;
    const unsigned full = nb & ~7u;
    if (bid < full) bid = (bid & 7u) * (full >> 3) + (bid >> 3);
    int b0 = 0, b1 = nbox - 1;
    while (b0 < b1) {
        const int mid = (b0 + b1 + 1) >> 1;
        if ((unsigned)start[mid] <= bid) b0 = mid; else b1 = mid - 1;
    }
    const DiffBoxDev B = tab[b0];
    unsigned t = bid - (unsigned)start[b0];
    const int ti = (int)(t % (unsigned)B.nt[0]);
    t /= (unsigned)B.nt[0];
    const int tj = (int)(t % (unsigned)B.nt[1]), tk = (int)(t / (unsigned)B.nt[1]);
    const int i = B.lo[0] + ti * 64 + (int)(threadIdx.x & 63u);
    const int j = B.lo[1] + tj * DIFF_TJ + (int)(threadIdx.x >> 6);
    if (i > B.hi[0] || j > B.hi[1]) return;
    const int k0 = B.lo[2] + tk * DIFF_KC;
    const int k1 = k0 + DIFF_KC - 1 < B.hi[2] ? k0 + DIFF_KC - 1 : B.hi[2];

    const bool pxl = D.phys_lo[0] && i == D.domlo[0], pxh = D.phys_hi[0] && i == D.domhi[0];
    const bool pyl = D.phys_lo[1] && j == D.domlo[1], pyh = D.phys_hi[1] && j == D.domhi[1];

    DiffColumn A, A2;
    A.start(B.U, D, i, j, k0);
    if (TWO) A2.start(B.U2, D, i, j, k0);
    double* __restrict__ se = B.Src.p ? B.Src.p + B.Src.sn * UEDEN : nullptr;
    double* __restrict__ si = B.Src.p ? B.Src.p + B.Src.sn * UEINT : nullptr;
    long cs = B.Src.p ? didx(B.Src, i, j, k0) : 0;
    long co = B.Out.p ? didx(B.Out, i, j, k0) : 0;
    for (int k = k0; k <= k1; ++k) {
        const bool pzl = D.phys_lo[2] && k == D.domlo[2], pzh = D.phys_hi[2] && k == D.domhi[2];
        const double d1 = A.term(D, pxl, pxh, pyl, pyh, pzl, pzh);
        A.advance();
        double d2 = 0.0;
        if (TWO) {
            d2 = A2.term(D, pxl, pxh, pyl, pyh, pzl, pzh);
            A2.advance();
        }
        if (se) {
            // MultiFab::Saxpy into UEDEN, then into UEINT (Castro_diffusion.cpp:91-94); the corrector adds its old-time half second
            double e = init ? 0.0 : se[cs], ei = init ? 0.0 : si[cs];
            e = e + m1 * d1;
            ei = ei + m1 * d1;
            if (TWO) {
                e = e + m2 * d2;
                ei = ei + m2 * d2;
            }
            se[cs] = e;
            si[cs] = ei;
            cs += B.Src.sz;
        }
        if (B.Out.p) {
            B.Out.p[co] = d1;
            co += B.Out.sz;
        }
    }
}

int launch_temp_diffusion(int nbox, DiffBoxDev* boxes, bool two, const DiffDev& D, double m1, double m2, int init,
                          StagedTable* arena, hipStream_t stream, Profiler* prof)
{
    if (nbox < 1 || !boxes || !arena) return 0;
    std::vector<int> start((size_t)nbox + 1, 0);
    for (int r = 0; r < nbox; ++r) {
        long n = 1;
        DiffBoxDev& B = boxes[r];
        const int per[3] = { 64, DIFF_TJ, DIFF_KC };
        for (int d = 0; d < 3; ++d) {
            const int ext = B.hi[d] - B.lo[d] + 1;
            B.nt[d] = ext > 0 ? (ext + per[d] - 1) / per[d] : 0;
            n *= B.nt[d];
        }
        if (start[(size_t)r] + n > 0x3fffffffL) return CASTRO_AMD_ERR_ARG;
        start[(size_t)r + 1] = start[(size_t)r] + (int)n;
    }
    if (start.back() <= 0) return 0;
    const DiffBoxDev* dbox;
    const int* dstart;
    const int rt = arena->stage(boxes, (size_t)nbox, start.data(), start.size(), stream, dbox, dstart);
    if (rt != 0) return rt;
    const unsigned nb = (unsigned)start.back();
    prof_begin(prof, two ? "k_temp_diffusion_corr" : "k_temp_diffusion", stream);
    if (two) hipLaunchKernelGGL(k_temp_diffusion<true>, dim3(nb), dim3(64 * DIFF_TJ), 0, stream, dbox, dstart, nbox, nb, D, m1, m2, init);
    else hipLaunchKernelGGL(k_temp_diffusion<false>, dim3(nb), dim3(64 * DIFF_TJ), 0, stream, dbox, dstart, nbox, nb, D, m1, m2, init);
    prof_end(prof, stream);
    return diff_launch_status();
}

// ---------------------------------------------------------------------------------------
// Castro::estdt_temp_diffusion (timestep.cpp:259-345): D = conductivity / (rho c_v) with the RAW conductivity (no scale
// factor, no ramp) and c_v = e / T of the gamma-law gas; zones at or below the cutoff density give max_dt / cfl.
// Wave shuffle -> LDS -> one atomic per block, like k_estdt.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_estdt_temp_diffusion(DFab U, int lo0, int lo1, int lo2, int n0, int n1, int n2,
                                                              double dx0, double dx1, double dx2, DevParams P, double cond,
                                                              double cutoff, double below, double* out)
{
    double dtmin = 1.e200;
    const long total = (long)n0 * n1 * n2;
    for (long tid = (long)blockIdx.x * blockDim.x + threadIdx.x; tid < total; tid += (long)gridDim.x * blockDim.x) {
        const int i = lo0 + (int)(tid % n0);
        const long rr = tid / n0;
        const int j = lo1 + (int)(rr % n1);
        const int k = lo2 + (int)(rr / n1);
        const long c = didx(U, i, j, k);
        const double rho = U.p[c + U.sn * URHO];
        double v = below;
        if (rho > cutoff) {
            const double rho_inv = 1.0 / rho;
            const double xn = U.p[c + U.sn * UFS] * rho_inv;
            const double cv = K_B / ((P.gamma - 1.0) * (eos_mu(P, xn) * M_U));
            const double Dc = cond * rho_inv / cv;
            const double dt1 = 0.5 * dx0 * dx0 / Dc;
            const double dt2 = 0.5 * dx1 * dx1 / Dc;
            const double dt3 = 0.5 * dx2 * dx2 / Dc;
            v = amin(amin(dt1, dt2), dt3);
        }
        dtmin = fmin(dtmin, v);              // a NaN zone is dropped, like in k_estdt
    }
    for (int off = 32; off > 0; off >>= 1) dtmin = fmin(dtmin, __shfl_down(dtmin, off, 64));
    __shared__ double sa[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sa[wave] = dtmin;
    __syncthreads();
    if (threadIdx.x == 0) atomic_min_double(out, fmin(fmin(sa[0], sa[1]), fmin(sa[2], sa[3])));
}

int launch_estdt_temp_diffusion(const DFab& U, const int lo[3], const int hi[3], const double dx[3], const DevParams& P,
                                double cond, double cutoff, double below, double* d_out, hipStream_t stream, Profiler* prof)
{
    long n = 1;
    int ext[3];
    for (int d = 0; d < 3; ++d) { ext[d] = hi[d] - lo[d] + 1; n *= ext[d] > 0 ? ext[d] : 0; }
    if (n <= 0) return 0;
    long nb = (n + 255) / 256;
    if (nb > 2048) nb = 2048;
    prof_begin(prof, "k_estdt_temp_diffusion", stream);
    hipLaunchKernelGGL(k_estdt_temp_diffusion, dim3((unsigned)nb), dim3(256), 0, stream, U, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2],
                       dx[0], dx[1], dx[2], P, cond, cutoff, below, d_out);
    prof_end(prof, stream);
    return diff_launch_status();
}

} // namespace cad

// checkpoint_kernels.hip -- the valid zones of many ghosted FABs into one contiguous buffer (castro_amd_fab_pack) and back
// (castro_amd_fab_unpack), with the minimum and maximum of every (FAB, component) reduced on the way: what a VisMF header lists.
//   k_fab_pack_minmax   one workgroup = one stretch of ONE component of ONE entry.  In the buffer a component's valid zones are
//                       contiguous (x fastest), so the stretch is a contiguous run of the buffer: the side that is written (pack)
//                       or read (unpack) is one unbroken stream, the FAB side is coalesced along the rows of the valid region.
//                       Where every row of the entry starts on a 16-byte boundary on both sides (torch allocations with an even
//                       row length, even ghost widths: the 256^3 level) a lane moves two zones per access, else one.  No wave
//                       straddles two entries or two components: its partial minimum / maximum belongs to one pair.  Every
//                       workgroup stores ONE (min, max) pair into the context's workspace.
//   k_fab_minmax_final  one thread per (entry, component) takes the pairs of its workgroups in order.
// No atomics, and comparisons instead of fmin / fmax: the same bits from the `exact` and the `contract` build.  A NaN in a valid
// zone PROPAGATES -- the minimum and the maximum of its (FAB, component) are NaN, as numpy's min / max and torch's amin / amax give
// them (the plotfile writer's host pass, the torch form of castro_amd/checkpoint.py): mm_min / mm_max take a NaN and then keep
// it, since no later value compares below or above it.  Of -0.0 and +0.0 the first one met stays.  A pure stream: every byte is
// read once, so the workgroup ids are taken as dealt.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "../../include/castro_hydro_amd.h"
#include "ctu_kernels.h"

namespace cad {

constexpr int PACK_WG = 256;              // 4 waves
constexpr int PACK_MAX_WG = 4096;         // a thread takes more items rather than the grid growing beyond it (256 CUs x 16)
enum { PACK_MINMAX = 0, PACK_COPY = 1, PACK_UNPACK = 2 };

// the running minimum / maximum with one more value: a NaN is taken and, once taken, stays (v < NaN and v > NaN are false)
__device__ __forceinline__ void mm_min(double v, double& mn) { if (v < mn || v != v) mn = v; }
__device__ __forceinline__ void mm_max(double v, double& mx) { if (v > mx || v != v) mx = v; }
__device__ __forceinline__ void mm_take(double v, double& mn, double& mx)
{
    mm_min(v, mn);
    mm_max(v, mx);
}

// start[e]: first workgroup of entry e; iters: items (zones, or pairs of zones) a thread takes
template <int MODE>
__global__ void __launch_bounds__(PACK_WG) k_fab_pack_minmax(const PackEntryDev* __restrict__ tab, const int* __restrict__ start, int n,
                                                            int iters, double* __restrict__ buf, double* __restrict__ ws)
{
    const unsigned bid = blockIdx.x;
    int e0 = 0, e1 = n - 1;
    while (e0 < e1) {
        const int mid = (e0 + e1 + 1) >> 1;
        if ((unsigned)start[mid] <= bid) e0 = mid; else e1 = mid - 1;
    }
    const PackEntryDev E = tab[e0];
    const unsigned local = bid - (unsigned)start[e0];
    const int c = (int)(local / (unsigned)E.bpc);
    const long chunk = (long)(local % (unsigned)E.bpc);
    const long items = E.items;                                 // per component
    double* __restrict__ fab = E.p + (long)c * E.sn;            // the first valid zone of component c
    double* __restrict__ lin = buf + E.offset + (long)c * E.zones;
    const long base = chunk * (long)PACK_WG * iters + threadIdx.x;
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();

    if (E.vec2) {
        const unsigned hx = (unsigned)(E.n[0] >> 1);            // pairs per row
        for (int it = 0; it < iters; ++it) {
            const long q = base + (long)it * PACK_WG;
            if (q >= items) break;
            const unsigned r = (unsigned)q / hx, i2 = (unsigned)q - r * hx;              // q < 2^31 (castro_amd_fab_pack checks)
            const unsigned k = r / (unsigned)E.n[1], j = r - k * (unsigned)E.n[1];
            double2* pf = reinterpret_cast<double2*>(fab + 2 * (long)i2 + E.sy * (long)j + E.sz * (long)k);
            double2* pl = reinterpret_cast<double2*>(lin + 2 * q);
            if (MODE == PACK_UNPACK) {
                *pf = *pl;
            } else {
                const double2 v = *pf;
                *pl = v;
                if (MODE == PACK_MINMAX) { mm_take(v.x, mn, mx); mm_take(v.y, mn, mx); }
            }
        }
    } else {
        const unsigned nx = (unsigned)E.n[0];
        for (int it = 0; it < iters; ++it) {
            const long q = base + (long)it * PACK_WG;
            if (q >= items) break;
            const unsigned r = (unsigned)q / nx, i = (unsigned)q - r * nx;
            const unsigned k = r / (unsigned)E.n[1], j = r - k * (unsigned)E.n[1];
            double* pf = fab + (long)i + E.sy * (long)j + E.sz * (long)k;
            if (MODE == PACK_UNPACK) {
                *pf = lin[q];
            } else {
                const double v = *pf;
                lin[q] = v;
                if (MODE == PACK_MINMAX) mm_take(v, mn, mx);
            }
        }
    }

    if (MODE == PACK_MINMAX) {
        // across the lanes of the wave, then across the four waves through LDS, each in a fixed order
        for (int off = 32; off > 0; off >>= 1) {
            const double a = __shfl_down(mn, off, 64), b = __shfl_down(mx, off, 64);
            mm_min(a, mn);
            mm_max(b, mx);
        }
        __shared__ double sm[PACK_WG / 64][2];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { sm[wave][0] = mn; sm[wave][1] = mx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < PACK_WG / 64; ++w) {
                mm_min(sm[w][0], mn);
                mm_max(sm[w][1], mx);
            }
            ws[2 * (long)bid] = mn;
            ws[2 * (long)bid + 1] = mx;
        }
    }
}

// rng[2 m], rng[2 m + 1]: the first workgroup and the number of workgroups of pair m = (entry, component); M pairs
__global__ void __launch_bounds__(PACK_WG) k_fab_minmax_final(const double* __restrict__ ws, const int* __restrict__ rng, int M,
                                                             double* __restrict__ minmax)
{
    const int m = (int)(blockIdx.x * (unsigned)PACK_WG + threadIdx.x);
    if (m >= M) return;
    const int first = rng[2 * m], count = rng[2 * m + 1];
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    for (int b = first; b < first + count; ++b) {
        const double a = ws[2 * (long)b], c = ws[2 * (long)b + 1];
        mm_min(a, mn);
        mm_max(c, mx);
    }
    minmax[m] = mn;
    minmax[M + m] = mx;
}

// the workgroups of every entry (bpc per component), the prefix over the entries and the ranges of the pairs
static int pack_layout(int n, PackEntryDev* tab, std::vector<int>& meta, int& iters, int& M)
{
    M = 0;
    for (int e = 0; e < n; ++e) M += tab[e].ncomp;
    long tot = 0;
    for (iters = 4; ; iters *= 2) {
        tot = 0;
        const long per = (long)PACK_WG * iters;
        for (int e = 0; e < n; ++e) {
            const long bpc = (tab[e].items + per - 1) / per;
            if (bpc > 0x3fffffffL) return CASTRO_AMD_ERR_ARG;
            tab[e].bpc = (int)bpc;
            tot += bpc * tab[e].ncomp;
        }
        if (tot <= PACK_MAX_WG || iters >= 4096) break;
    }
    if (tot >= 0x3fffffffL) return CASTRO_AMD_ERR_ARG;
    // meta: start[0 .. n], then at the next even index (first, count) of every pair
    meta.assign((size_t)n + 1 + ((n + 1) & 1) + 2 * (size_t)M, 0);
    int at = 0, m = 0;
    const size_t r0 = (size_t)n + 1 + ((n + 1) & 1);
    for (int e = 0; e < n; ++e) {
        meta[(size_t)e] = at;
        for (int c = 0; c < tab[e].ncomp; ++c, ++m) {
            meta[r0 + 2 * (size_t)m] = at + c * tab[e].bpc;
            meta[r0 + 2 * (size_t)m + 1] = tab[e].bpc;
        }
        at += tab[e].bpc * tab[e].ncomp;
    }
    meta[(size_t)n] = at;
    return 0;
}

int launch_fab_pack(int mode, int n, PackEntryDev* tab, StagedTable* arena, DiagWorkspace* ws, double* buf, double* d_minmax,
                    hipStream_t stream, Profiler* prof)
{
    if (n <= 0) return 0;
    std::vector<int> meta;
    int iters = 4, M = 0;
    const int rc = pack_layout(n, tab, meta, iters, M);
    if (rc != 0) return rc;
    const int nb = meta[(size_t)n];
    if (nb <= 0) return 0;
    const bool minmax = mode == 0 && d_minmax != nullptr;
    if (minmax && (size_t)nb > ws->rows) {
        const size_t rows = (size_t)nb > 2 * (size_t)PACK_MAX_WG ? (size_t)nb : 2 * (size_t)PACK_MAX_WG;
        if (ws->p) { (void)hipStreamSynchronize(stream); (void)hipFree(ws->p); ws->p = nullptr; ws->rows = 0; }
        if (hipMalloc(&ws->p, rows * 2 * sizeof(double)) != hipSuccess) return CASTRO_AMD_ERR_NOMEM;
        ws->rows = rows;
    }
    const PackEntryDev* dtab;
    const int* dmeta;
    const int rt = arena->stage(tab, (size_t)n, meta.data(), meta.size(), stream, dtab, dmeta);
    if (rt != 0) return rt;
    const dim3 grid((unsigned)nb), block(PACK_WG);
    if (mode != 0) {
        prof_begin(prof, "k_fab_unpack", stream);
        hipLaunchKernelGGL(k_fab_pack_minmax<PACK_UNPACK>, grid, block, 0, stream, dtab, dmeta, n, iters, buf, (double*)nullptr);
    } else if (minmax) {
        prof_begin(prof, "k_fab_pack_minmax", stream);
        hipLaunchKernelGGL(k_fab_pack_minmax<PACK_MINMAX>, grid, block, 0, stream, dtab, dmeta, n, iters, buf, ws->p);
    } else {
        prof_begin(prof, "k_fab_pack", stream);
        hipLaunchKernelGGL(k_fab_pack_minmax<PACK_COPY>, grid, block, 0, stream, dtab, dmeta, n, iters, buf, (double*)nullptr);
    }
    prof_end(prof, stream);
    if (hipGetLastError() != hipSuccess) return CASTRO_AMD_ERR_HIP;
    if (minmax) {
        const size_t r0 = (size_t)n + 1 + ((n + 1) & 1);
        prof_begin(prof, "k_fab_minmax_final", stream);
        hipLaunchKernelGGL(k_fab_minmax_final, dim3((unsigned)((M + PACK_WG - 1) / PACK_WG)), block, 0, stream,
                           (const double*)ws->p, dmeta + r0, M, d_minmax);
        prof_end(prof, stream);
        if (hipGetLastError() != hipSuccess) return CASTRO_AMD_ERR_HIP;
    }
    return 0;
}

} // namespace cad

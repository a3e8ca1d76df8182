// diag_kernels.hip -- the integrated quantities of Castro::sum_integrated_quantities (Source/driver/sum_integrated_quantities.cpp:60-230;
// volWgtSum / locWgtSum, sum_utils.cpp:17-205) for every box of a level in one call:
//   k_diag_partial  every workgroup sums CASTRO_AMD_DIAG_N = 14 quantities over its share of the valid zones and stores ONE row
//                   of 14 doubles into the context's workspace
//   k_diag_final    one workgroup adds the rows in a fixed order and overwrites d_out[0..13]
// No floating-point atomics: the order of every addition is a function of the box table alone (and of the 16-byte alignment
// of the rows), so the same boxes give the same bits on every call and on every stream -- an atomic sum depends on the order
// in which the workgroups arrive.  The kernel is a pure stream (every byte is read once, nothing is reused), so the workgroup
// ids are taken as they are dealt: there is no neighbour whose lines an XCD's L2 could keep.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "../../include/castro_hydro_amd.h"
#include "hydro_device.h"
#include "ctu_kernels.h"

namespace cad {

constexpr int DIAG_N = CASTRO_AMD_DIAG_N;
constexpr int DIAG_WG = 256;              // threads of a k_diag_partial workgroup: 4 waves
constexpr int DIAG_MAX_WG = 2048;         // 256 CUs x 8 workgroups: a thread takes more pairs rather than the grid growing beyond it
constexpr int DIAG_FINAL_WG = 1024;       // k_diag_final: 64 groups of rows x 16 columns (14 used)

// The terms of one zone.  kineng and the angular momentum are the expressions of k_derive (aux_kernels.hip, cases 1 and 22-24)
// restated: in the `exact` build (no contraction) they are the bits of the derived fields.
struct DiagZone { double rho, mx, my, mz, eden, eint, rx; };

__device__ __forceinline__ void diag_add(double (&s)[DIAG_N], const DiagZone& z, const DiagGeom& G, int i, int j, int k)
{
    const double vol = G.vol;
    const double x0 = G.problo[0] + (0.5 + (double)i) * G.dx[0];
    const double x1 = G.problo[1] + (0.5 + (double)j) * G.dx[1];
    const double x2 = G.problo[2] + (0.5 + (double)k) * G.dx[2];
    double loc0 = x0, loc1 = x1, loc2 = x2;
    loc0 -= G.center[0]; loc1 -= G.center[1]; loc2 -= G.center[2];
    s[CASTRO_AMD_DIAG_MASS] += z.rho * vol;
    s[CASTRO_AMD_DIAG_XMOM] += z.mx * vol;
    s[CASTRO_AMD_DIAG_YMOM] += z.my * vol;
    s[CASTRO_AMD_DIAG_ZMOM] += z.mz * vol;
    s[CASTRO_AMD_DIAG_ANGMOM_X] += (loc1 * z.mz - loc2 * z.my) * vol;
    s[CASTRO_AMD_DIAG_ANGMOM_Y] += (loc2 * z.mx - loc0 * z.mz) * vol;
    s[CASTRO_AMD_DIAG_ANGMOM_Z] += (loc0 * z.my - loc1 * z.mx) * vol;
    s[CASTRO_AMD_DIAG_RHO_E_INT] += z.eint * vol;
    s[CASTRO_AMD_DIAG_RHO_K] += (0.5 / z.rho * (z.mx * z.mx + z.my * z.my + z.mz * z.mz)) * vol;
    s[CASTRO_AMD_DIAG_RHO_E] += z.eden * vol;
    s[CASTRO_AMD_DIAG_COM_X] += (z.rho * x0) * vol;
    s[CASTRO_AMD_DIAG_COM_Y] += (z.rho * x1) * vol;
    s[CASTRO_AMD_DIAG_COM_Z] += (z.rho * x2) * vol;
    s[CASTRO_AMD_DIAG_SPECIES] += z.rx * vol;
}

// two x-adjacent zones of one component: one 16-byte load where both are wanted and the address allows it, else only the
// zones that are wanted (a zone that is not wanted may be a ghost zone, or lie outside the FAB: it is never loaded)
__device__ __forceinline__ void diag_load2(const double* __restrict__ p, bool a, bool b, double& va, double& vb)
{
    if (a && b && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const double2 v = *reinterpret_cast<const double2*>(p);
        va = v.x; vb = v.y;
    } else {
        va = a ? p[0] : 0.0;
        vb = b ? p[1] : 0.0;
    }
}

__global__ void __launch_bounds__(DIAG_WG) k_diag_partial(const DiagBoxDev* __restrict__ tab, const int* __restrict__ start, int nbox,
                                                          int iters, DiagGeom G, double* __restrict__ ws)
{
    const unsigned bid = blockIdx.x;
    int b0 = 0, b1 = nbox - 1;
    while (b0 < b1) {
        const int mid = (b0 + b1 + 1) >> 1;
        if ((unsigned)start[mid] <= bid) b0 = mid; else b1 = mid - 1;
    }
    const DiagBoxDev B = tab[b0];
    const long total = (long)B.npr * B.n[1] * B.n[2];
    const long base = (long)(bid - (unsigned)start[b0]) * DIAG_WG * iters + threadIdx.x;
    const int hi0 = B.lo[0] + B.n[0] - 1;

    double s[DIAG_N];
#pragma unroll
    for (int m = 0; m < DIAG_N; ++m) s[m] = 0.0;

    for (int it = 0; it < iters; ++it) {
        const long q = base + (long)it * DIAG_WG;
        if (q >= total) break;
        const int pq = (int)(q % B.npr);
        const long r = q / B.npr;
        const int jj = (int)(r % B.n[1]), kk = (int)(r / B.n[1]);
        const int j = B.lo[1] + jj, k = B.lo[2] + kk;
        // the pairs of a row start at an even distance from a 16-byte boundary of component 0: where the row itself starts at
        // an odd one, its first pair is the zone in front of the row (not read) and the first zone
        const double* __restrict__ row = B.U.p + (long)(B.lo[0] - B.U.lo[0]) + B.U.sy * (long)(j - B.U.lo[1]) + B.U.sz * (long)(k - B.U.lo[2]);
        const int phase = (int)((reinterpret_cast<uintptr_t>(row) >> 3) & 1u);
        const int ia = B.lo[0] - phase + 2 * pq;
        bool oka = ia >= B.lo[0] && ia <= hi0, okb = ia + 1 <= hi0;
        if (B.mask) {
            const unsigned char* __restrict__ mrow = B.mask + (long)B.n[0] * ((long)jj + (long)B.n[1] * kk);
            if (oka) oka = mrow[ia - B.lo[0]] != 0;
            if (okb) okb = mrow[ia + 1 - B.lo[0]] != 0;
        }
        if (!oka && !okb) continue;
        const double* __restrict__ p = row + (ia - B.lo[0]);
        DiagZone za, zb;
        diag_load2(p + B.U.sn * URHO, oka, okb, za.rho, zb.rho);
        diag_load2(p + B.U.sn * UMX, oka, okb, za.mx, zb.mx);
        diag_load2(p + B.U.sn * UMY, oka, okb, za.my, zb.my);
        diag_load2(p + B.U.sn * UMZ, oka, okb, za.mz, zb.mz);
        diag_load2(p + B.U.sn * UEDEN, oka, okb, za.eden, zb.eden);
        diag_load2(p + B.U.sn * UEINT, oka, okb, za.eint, zb.eint);
        diag_load2(p + B.U.sn * UFS, oka, okb, za.rx, zb.rx);
        if (oka) diag_add(s, za, G, ia, j, k);
        if (okb) diag_add(s, zb, G, ia + 1, j, k);
    }

    // across the lanes of the wave, then across the four waves through LDS, each in a fixed order
#pragma unroll
    for (int m = 0; m < DIAG_N; ++m)
        for (int off = 32; off > 0; off >>= 1) s[m] += __shfl_down(s[m], off, 64);
    __shared__ double sa[DIAG_WG / 64][DIAG_N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < DIAG_N; ++m) sa[wave][m] = s[m];
    }
    __syncthreads();
    if (threadIdx.x < DIAG_N) {
        const int m = threadIdx.x;
        ws[(long)bid * DIAG_N + m] = ((sa[0][m] + sa[1][m]) + sa[2][m]) + sa[3][m];
    }
}

// rows g, g + 64, g + 128, ... by group g, then the 64 groups pairwise (32, 16, ... 1): an order fixed by nrows alone
__global__ void __launch_bounds__(DIAG_FINAL_WG) k_diag_final(const double* __restrict__ ws, int nrows, double* __restrict__ out)
{
    __shared__ double sg[DIAG_FINAL_WG / 16][16];
    const int col = threadIdx.x & 15, grp = threadIdx.x >> 4;
    double acc = 0.0;
    if (col < DIAG_N)
        for (int r = grp; r < nrows; r += DIAG_FINAL_WG / 16) acc += ws[(long)r * DIAG_N + col];
    sg[grp][col] = acc;
    __syncthreads();
    for (int stride = DIAG_FINAL_WG / 32; stride > 0; stride >>= 1) {
        if (grp < stride) sg[grp][col] += sg[grp + stride][col];
        __syncthreads();
    }
    if (grp == 0 && col < DIAG_N) out[col] = sg[0][col];
}

int diag_layout(int nbox, DiagBoxDev* boxes, std::vector<int>& start, int& iters)
{
    start.assign((size_t)nbox + 1, 0);
    std::vector<long> units((size_t)nbox, 0);
    for (int r = 0; r < nbox; ++r) {
        DiagBoxDev& B = boxes[r];
        if (B.n[0] <= 0 || B.n[1] <= 0 || B.n[2] <= 0) { B.npr = 0; continue; }
        // does any row start at an odd distance from a 16-byte boundary?  With even strides all rows are alike
        const long odd0 = (long)((reinterpret_cast<uintptr_t>(B.U.p) >> 3) & 1u) + (B.lo[0] - B.U.lo[0]);
        const bool alike = (B.U.sy % 2 == 0) && (B.U.sz % 2 == 0);
        const int shift = alike ? (int)(odd0 & 1) : 1;
        B.npr = (B.n[0] + shift + 1) / 2;
        units[(size_t)r] = (long)B.npr * B.n[1] * B.n[2];
    }
    for (iters = 4; ; iters *= 2) {
        long tot = 0;
        for (int r = 0; r < nbox; ++r) {
            const long per = (long)DIAG_WG * iters;
            tot += (units[(size_t)r] + per - 1) / per;
            start[(size_t)r + 1] = (int)(tot < 0x3fffffffL ? tot : 0x3fffffffL);
        }
        if (tot <= DIAG_MAX_WG || iters >= 4096) {
            if (tot >= 0x3fffffffL) return CASTRO_AMD_ERR_ARG;
            break;
        }
    }
    return 0;
}

int launch_integrated_quantities(int nbox, DiagBoxDev* boxes, const DiagGeom& G, StagedTable* arena, DiagWorkspace* ws,
                                 double* d_out, hipStream_t stream, Profiler* prof)
{
    std::vector<int> start;
    int iters = 4;
    if (nbox > 0) {
        const int rc = diag_layout(nbox, boxes, start, iters);
        if (rc != 0) return rc;
    }
    const int nb = nbox > 0 ? start.back() : 0;
    if (nb > 0) {
        if ((size_t)nb > ws->rows) {
            const size_t rows = (size_t)nb > 2 * (size_t)DIAG_MAX_WG ? (size_t)nb : 2 * (size_t)DIAG_MAX_WG;
            if (ws->p) { (void)hipStreamSynchronize(stream); (void)hipFree(ws->p); ws->p = nullptr; ws->rows = 0; }
            if (hipMalloc(&ws->p, rows * DIAG_N * sizeof(double)) != hipSuccess) return CASTRO_AMD_ERR_NOMEM;
            ws->rows = rows;
        }
        const DiagBoxDev* dbox;
        const int* dstart;
        const int rt = arena->stage(boxes, (size_t)nbox, start.data(), start.size(), stream, dbox, dstart);
        if (rt != 0) return rt;
        prof_begin(prof, "k_diag_partial", stream);
        hipLaunchKernelGGL(k_diag_partial, dim3((unsigned)nb), dim3(DIAG_WG), 0, stream, dbox, dstart, nbox, iters, G, ws->p);
        prof_end(prof, stream);
        if (hipGetLastError() != hipSuccess) return CASTRO_AMD_ERR_HIP;
    }
    prof_begin(prof, "k_diag_final", stream);
    hipLaunchKernelGGL(k_diag_final, dim3(1), dim3(DIAG_FINAL_WG), 0, stream, (const double*)ws->p, nb, d_out);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

} // namespace cad

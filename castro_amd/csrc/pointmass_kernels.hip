// pointmass_kernels.hip -- the central point mass of the gravity module (castro.use_point_mass, castro.point_mass,
// castro.point_mass_fix_solution), 3-D Cartesian:
//   k_add_pointmass      Gravity::add_pointmass_to_gravity (Source/gravity/Gravity.cpp:2903-2948, without the phi part) over the
//                        whole box -- ghost zones included -- of every gravity FAB of a table, one launch
//   k_pointmass_delta    the mass sum of Castro::pointmass_update (Source/gravity/Castro_pointmass.cpp:20-86): vol * (rho_new -
//                        rho_old) over the 4 x 4 x 4 zones around the centre, clipped to the boxes of a table
//   k_pointmass_apply    its second half (:88-153): where the summed change is positive, point_mass += change and the cube zones
//                        of S_new take all NUM_STATE components of S_old
// The point mass is read from (and, by k_pointmass_apply, added to) ONE device double, and the mass change travels in another:
// delta -> sum over the ranks -> apply is a sequence of stream-ordered launches without a host round trip.
//
// Numerics.  `exact` build (-ffp-contract=off): the expressions of the reference in its order -- x*x + y*y + z*z left to right,
// -Gconst * M / rsq, 1 / sqrt(rsq), grav += radial_force * (x * rinv) -- with IEEE division and sqrt: the bits of the numpy
// restatement (tests/pointmass_ref.py).  `contract` build: the same source under the build's flags (FMA contraction).
//
// The order of the mass sum (no floating-point atomics).  The cube has at most 64 zones: ONE wave, lane l owns the cube zone
// (l & 3, (l >> 2) & 3, l >> 4) counted from the cube's low corner, looks its zone up in the box table (the boxes of a level are
// disjoint: the first box that holds it) and forms its term, 0 where no box of the table holds the zone.  Lane 0 adds the 64
// terms in lane order.  The order is a function of the zone index alone -- the same bits for any cut of the level into boxes, on
// every call and on every stream.
#include <hip/hip_runtime.h>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../include/castro_hydro_amd.h"
#include "hydro_device.h"
#include "ctu_kernels.h"

namespace cad {

// one thread per zone of the table: FAB b holds the zones [start[b], start[b + 1]) of the launch
__global__ void __launch_bounds__(256) k_add_pointmass(const PmFabDev* __restrict__ tab, int nfab, long ntot, PmGeom G,
                                                       const double* __restrict__ d_mass)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= ntot) return;
    int b0 = 0, b1 = nfab - 1;
    while (b0 < b1) {
        const int mid = (b0 + b1 + 1) >> 1;
        if (tab[mid].start <= tid) b0 = mid; else b1 = mid - 1;
    }
    const PmFabDev B = tab[b0];
    const long t = tid - B.start;
    const int i = B.lo[0] + (int)(t % B.n[0]);
    const long rr = t / B.n[0];
    const int j = B.lo[1] + (int)(rr % B.n[1]), k = B.lo[2] + (int)(rr / B.n[1]);
    const double M = *d_mass;

    const double x = G.problo[0] + ((double)i + 0.5) * G.dx[0] - G.center[0];
    const double y = G.problo[1] + ((double)j + 0.5) * G.dx[1] - G.center[1];
    const double z = G.problo[2] + ((double)k + 0.5) * G.dx[2] - G.center[2];
    const double rsq = x * x + y * y + z * z;
    const double radial_force = -G.Gconst * M / rsq;
    const double rinv = 1.e0 / sqrt(rsq);

    double* p = B.F.p + ((long)(i - B.F.lo[0]) + B.F.sy * (long)(j - B.F.lo[1]) + B.F.sz * (long)(k - B.F.lo[2]));
    p[0] += radial_force * (x * rinv);
    p[B.F.sn] += radial_force * (y * rinv);
    p[2 * B.F.sn] += radial_force * (z * rinv);
}

// the box of the table that holds zone (i, j, k), or -1
__device__ __forceinline__ int pm_find_box(const PmBoxDev* __restrict__ tab, int nbox, int i, int j, int k)
{
    for (int b = 0; b < nbox; ++b) {
        const PmBoxDev& B = tab[b];
        if (i >= B.lo[0] && i <= B.hi[0] && j >= B.lo[1] && j <= B.hi[1] && k >= B.lo[2] && k <= B.hi[2]) return b;
    }
    return -1;
}

__device__ __forceinline__ long pm_index(const DFab& F, int i, int j, int k)
{
    return (long)(i - F.lo[0]) + F.sy * (long)(j - F.lo[1]) + F.sz * (long)(k - F.lo[2]);
}

// one wave; cube = [clo, clo + 3]^3
__global__ void __launch_bounds__(64) k_pointmass_delta(const PmBoxDev* __restrict__ tab, int nbox, int clo0, int clo1, int clo2,
                                                        double vol, double* __restrict__ d_delta)
{
    __shared__ double term[64];
    const int l = threadIdx.x;
    const int i = clo0 + (l & 3), j = clo1 + ((l >> 2) & 3), k = clo2 + (l >> 4);
    const int b = pm_find_box(tab, nbox, i, j, k);
    double t = 0.0;
    if (b >= 0) {
        const PmBoxDev& B = tab[b];
        const double rn = B.Sn.p[pm_index(B.Sn, i, j, k) + B.Sn.sn * URHO];
        const double ro = B.So.p[pm_index(B.So, i, j, k) + B.So.sn * URHO];
        t = vol * (rn - ro);
    }
    term[l] = t;
    __syncthreads();
    if (l == 0) {
        double s = 0.0;
        for (int q = 0; q < 64; ++q) s += term[q];
        *d_delta = s;
    }
}

__global__ void __launch_bounds__(64) k_pointmass_apply(const PmBoxDev* __restrict__ tab, int nbox, int clo0, int clo1, int clo2,
                                                        const double* __restrict__ d_delta, double* __restrict__ d_mass)
{
    const double delta = *d_delta;
    if (!(delta > 0.0)) return;
    const int l = threadIdx.x;
    const int i = clo0 + (l & 3), j = clo1 + ((l >> 2) & 3), k = clo2 + (l >> 4);
    const int b = pm_find_box(tab, nbox, i, j, k);
    if (b >= 0) {
        const PmBoxDev& B = tab[b];
        const long cn = pm_index(B.Sn, i, j, k), co = pm_index(B.So, i, j, k);
        for (int n = 0; n < NUM_STATE; ++n) B.Sn.p[cn + B.Sn.sn * n] = B.So.p[co + B.So.sn * n];
    }
    if (l == 0) *d_mass = *d_mass + delta;
}

// The tables are kept on the device per content (TableCache, dev_table.h): fully initialised bytes

int launch_add_pointmass(int nfab, PmFabDev* fabs, const PmGeom& G, const double* d_mass, TableCache* tables, hipStream_t stream,
                         Profiler* prof)
{
    long tot = 0;
    for (int b = 0; b < nfab; ++b) {
        PmFabDev& B = fabs[b];
        if (B.n[0] <= 0 || B.n[1] <= 0 || B.n[2] <= 0) return CASTRO_AMD_ERR_ARG;
        B.start = tot;
        tot += (long)B.n[0] * B.n[1] * B.n[2];
    }
    if (nfab == 0 || tot == 0) return 0;
    if ((tot + 255) / 256 >= 0x7fffffffL) return CASTRO_AMD_ERR_ARG;
    const PmFabDev* dtab = nullptr;
    const int rt = tables->find(fabs, (size_t)nfab, stream, dtab);
    if (rt != 0) return rt;
    prof_begin(prof, "k_add_pointmass", stream);
    hipLaunchKernelGGL(k_add_pointmass, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, dtab, nfab, tot, G, d_mass);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

// nbox == 0 (a rank without a box of the level): the delta is 0, the apply only adds the summed change to the point mass
int launch_pointmass_delta(int nbox, const PmBoxDev* boxes, const int clo[3], double vol, double* d_delta, TableCache* tables,
                           hipStream_t stream, Profiler* prof)
{
    const PmBoxDev* dtab = nullptr;
    if (nbox > 0) {
        const int rt = tables->find(boxes, (size_t)nbox, stream, dtab);
        if (rt != 0) return rt;
    }
    prof_begin(prof, "k_pointmass_delta", stream);
    hipLaunchKernelGGL(k_pointmass_delta, dim3(1), dim3(64), 0, stream, dtab, nbox, clo[0], clo[1], clo[2], vol, d_delta);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

int launch_pointmass_apply(int nbox, const PmBoxDev* boxes, const int clo[3], const double* d_delta, double* d_mass,
                           TableCache* tables, hipStream_t stream, Profiler* prof)
{
    const PmBoxDev* dtab = nullptr;
    if (nbox > 0) {
        const int rt = tables->find(boxes, (size_t)nbox, stream, dtab);
        if (rt != 0) return rt;
    }
    prof_begin(prof, "k_pointmass_apply", stream);
    hipLaunchKernelGGL(k_pointmass_apply, dim3(1), dim3(64), 0, stream, dtab, nbox, clo[0], clo[1], clo[2], d_delta, d_mass);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

} // namespace cad

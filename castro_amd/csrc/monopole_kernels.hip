// monopole_kernels.hip -- gravity.gravity_type = "MonopoleGrav" (Source/gravity/Gravity.cpp), 3-D Cartesian:
//   k_radial_partial + k_radial_final   Gravity::compute_radial_mass (:1409-1576): the radial histogram of mass and volume;
//                                       k_radial_partial<true, MonoBoxDevEx>: of a state between two time levels (:2987-3000)
//   k_radial_combine                    the level combination of make_radial_gravity (:3103-3168)
//   k_grav_bc_fill                      the physical-boundary fill of Gravity_Type (Castro_setup.cpp:614-622)
//   k_radial_gravity                    the outward integration of make_radial_gravity (:3170-3274, no GR_GRAV)
//   k_monopole_grav                     interpolate_monopole_grav (:1300-1406) onto a grown 3-component gravity FAB
// Everything here is compiled with contraction off in BOTH builds (the Makefile gives this file -ffp-contract=off in the
// `contract` build: under -ffp-contract=fast the back end fuses whatever the pragma below says, which alone only serves a
// build with fast-honor-pragmas): the bin of a sub-zone is a discrete
// switch, (int)(r * drinv), and must be the same in the `exact` build, the `contract` build and the numpy restatement of the
// tests; the integration is n1d sequential iterations and the interpolation a handful of operations per zone, so the
// `contract` build would gain nothing by differing.
//
// The order of the mass sums (no floating-point atomics).  k_radial_partial: one workgroup of 4 waves takes a fixed brick of
// 8 x 8 x 4 zones of one box (one zone per thread, wave w the x-y plane w of the brick).  All sub-zones of the brick fall into a
// window of 64 bins that starts at `base`, one bin below the bin of the point of the brick nearest to the centre
// (castro_amd_radial_mass_mf refuses a drdxfac whose bricks span more: radial_window_ok).  Lane l of every wave owns bin
// base + l.  For every sub-zone (kk, jj, ii in the reference's loop order) the wave walks its lanes in lane order, and the owner
// of the lane's bin adds the lane's term: a bin receives its terms in the order (sub-zone, lane).  The four waves are added
// through LDS in wave order and the workgroup stores the window as ONE row of 64 doubles of the context's workspace, with its
// base.  k_radial_final: for every bin, 16 groups of consecutive rows are added in row order each, then the groups in group
// order, and the result OVERWRITES the output.  Every one of these orders is a function of the box table (and n1d) alone, so
// the same boxes give the same bits on every call and on every stream -- the property diag_kernels.hip documents.
// Volumes: the reference adds vol_frac to radial_vol[index] once per sub-zone; here the sub-zones of a bin are COUNTED (integer
// atomics: exact, order-free) and radial_vol[i] = count[i] * vol_frac is formed once in k_radial_final.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../include/castro_hydro_amd.h"
#include "hydro_device.h"
#include "ctu_kernels.h"

#pragma clang fp contract(off)

namespace cad {

constexpr int MONO_BX = 8, MONO_BY = 8, MONO_BZ = 4;        // zones of a brick: MONO_BZ waves of MONO_BX x MONO_BY lanes
constexpr int MONO_WG = MONO_BX * MONO_BY * MONO_BZ;
constexpr int MONO_WIN = 64;                                // bins of a window: one per lane
constexpr int MONO_FINAL_GROUPS = 16;
static_assert(MONO_BX * MONO_BY == 64 && MONO_WG == 256, "a wave is one x-y plane of the brick");

// distance from 0 to the interval [a, b]
__host__ __device__ inline double mono_near(double a, double b) { return a > 0.0 ? a : (b < 0.0 ? -b : 0.0); }
__host__ __device__ inline double mono_far(double a, double b) { return fabs(a) > fabs(b) ? fabs(a) : fabs(b); }

// Does every brick of any box keep its sub-zones inside a window of MONO_WIN bins?  The bins of a brick span at most
// (its diagonal) / dr, plus one bin below (the base) and two for the truncations and the rounding of r
bool radial_window_ok(const MonoGeom& G)
{
    const double dr = G.dx[0] / (double)G.drdxfac;
    const double ex = MONO_BX * G.dx[0], ey = MONO_BY * G.dx[1], ez = MONO_BZ * G.dx[2];
    return std::sqrt(ex * ex + ey * ey + ez * ez) / dr + 3.0 <= (double)MONO_WIN;
}

__device__ __forceinline__ double mono_readlane(double v, int s)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), s);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), s);
    return __hiloint2double(hi, lo);
}

// The body of the binning kernels.  INTERP = false (BOX = MonoBoxDev): the density of a zone is U(URHO).  INTERP = true
// (BOX = MonoBoxDevEx): the state of a coarser level between its two time levels (Gravity.cpp:2987-3000, S = S_old * omalpha,
// S_new * alpha, S = S + S_new): rho = (rho_old * omalpha) + (rho_new * alpha), the two products rounded, then the sum -- this
// file is compiled without contraction --, and the rho == 0 test of :1491 is made on that value.
template <bool INTERP, class BOX>
__global__ void __launch_bounds__(MONO_WG) k_radial_partial(const BOX* __restrict__ tab, const int* __restrict__ start, int nbox,
                                                           MonoGeom G, double* __restrict__ rows, int* __restrict__ rbase,
                                                           unsigned long long* __restrict__ count)
{
    const unsigned bid = blockIdx.x;
    int b0 = 0, b1 = nbox - 1;
    while (b0 < b1) {
        const int mid = (b0 + b1 + 1) >> 1;
        if ((unsigned)start[mid] <= bid) b0 = mid; else b1 = mid - 1;
    }
    const BOX B = tab[b0];
    const int lb = (int)(bid - (unsigned)start[b0]);
    const int bx = lb % B.nb[0], by = (lb / B.nb[0]) % B.nb[1], bz = lb / (B.nb[0] * B.nb[1]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = B.lo[0] + MONO_BX * bx, j0 = B.lo[1] + MONO_BY * by, k0 = B.lo[2] + MONO_BZ * bz;
    const int i = i0 + (lane & (MONO_BX - 1)), j = j0 + (lane / MONO_BX), k = k0 + wave;

    const double dr = G.dx[0] / (double)G.drdxfac;
    const double drinv = 1.0 / dr;
    const int n1d = G.n1d;

    // the window of the brick (the same in its four waves): one bin below the bin of its nearest point
    int base;
    {
        const double xa = G.problo[0] + (double)i0 * G.dx[0] - G.center[0], xb = G.problo[0] + (double)(i0 + MONO_BX) * G.dx[0] - G.center[0];
        const double ya = G.problo[1] + (double)j0 * G.dx[1] - G.center[1], yb = G.problo[1] + (double)(j0 + MONO_BY) * G.dx[1] - G.center[1];
        const double za = G.problo[2] + (double)k0 * G.dx[2] - G.center[2], zb = G.problo[2] + (double)(k0 + MONO_BZ) * G.dx[2] - G.center[2];
        const double nx = mono_near(xa, xb), ny = mono_near(ya, yb), nz = mono_near(za, zb);
        const double q = sqrt(nx * nx + ny * ny + nz * nz) * drinv;
        base = q < 2.0e9 ? (int)q - 1 : 2000000000;
        if (base < 0) base = 0;
    }

    bool ok = i < B.lo[0] + B.n[0] && j < B.lo[1] + B.n[1] && k < B.lo[2] + B.n[2];
    if (ok && B.mask)
        ok = B.mask[(long)(i - B.lo[0]) + (long)B.n[0] * ((long)(j - B.lo[1]) + (long)B.n[1] * (k - B.lo[2]))] != 0;
    double rho = 0.0;
    if (ok) {
        rho = B.U.p[(long)(i - B.U.lo[0]) + B.U.sy * (long)(j - B.U.lo[1]) + B.U.sz * (long)(k - B.U.lo[2]) + B.U.sn * URHO];
        if constexpr (INTERP) {
            const double rho_new = B.U2.p[(long)(i - B.U2.lo[0]) + B.U2.sy * (long)(j - B.U2.lo[1]) + B.U2.sz * (long)(k - B.U2.lo[2]) + B.U2.sn * URHO];
            const double so = rho * B.omalpha, sn = rho_new * B.alpha;
            rho = so + sn;
        }
        ok = rho != 0.0;                                  // a zone masked out by a zeroed density (:1491)
    }

    // the expressions of :1474-1484, 1459-1463
    const double xc = G.problo[0] + ((double)i + 0.5) * G.dx[0] - G.center[0];
    const double lo_i = G.problo[0] + (double)i * G.dx[0] - G.center[0];
    const double yc = G.problo[1] + ((double)j + 0.5) * G.dx[1] - G.center[1];
    const double lo_j = G.problo[1] + (double)j * G.dx[1] - G.center[1];
    const double zc = G.problo[2] + ((double)k + 0.5) * G.dx[2] - G.center[2];
    const double lo_k = G.problo[2] + (double)k * G.dx[2] - G.center[2];
    {
        const double r = sqrt(xc * xc + yc * yc + zc * zc);
        const double q = r * drinv;
        // the whole zone is dropped when its centre lies beyond the last bin (:1514)
        if (!(q < 2.0e9) || (int)q > n1d - 1) ok = false;
    }
    const double fac = (double)G.drdxfac;
    const double dx_frac = G.dx[0] / fac, dy_frac = G.dx[1] / fac, dz_frac = G.dx[2] / fac;
    const double vol_frac = G.octant_factor * dx_frac * dy_frac * dz_frac;
    const double term = vol_frac * rho;

    double acc = 0.0;
    int cnt = 0;
    const int nsub = G.drdxfac;
    for (int kk = 0; kk < nsub; ++kk) {
        const double zz = lo_k + ((double)kk + 0.5) * dz_frac;
        const double zzsq = zz * zz;
        for (int jj = 0; jj < nsub; ++jj) {
            const double yy = lo_j + ((double)jj + 0.5) * dy_frac;
            const double yysq = yy * yy;
            for (int ii = 0; ii < nsub; ++ii) {
                const double xx = lo_i + ((double)ii + 0.5) * dx_frac;
                const double xxsq = xx * xx;
                const double r = sqrt(xxsq + yysq + zzsq);
                const double q = r * drinv;
                int rel = -1;
                if (ok && q < 2.0e9) {
                    const int index = (int)q;
                    if (index <= n1d - 1) rel = index - base;        // outside [0, MONO_WIN): no owner (radial_window_ok rules it out)
                }
                // the lanes with a term, in lane order: the owner of the lane's bin adds it
                unsigned long long m = __ballot(rel >= 0);
                while (m) {
                    const int s = __builtin_ctzll(m);
                    m &= m - 1;
                    const int rs = __builtin_amdgcn_readlane(rel, s);
                    const double ts = mono_readlane(term, s);
                    if (rs == lane) { acc += ts; cnt += 1; }
                }
            }
        }
    }

    __shared__ double sa[MONO_BZ][MONO_WIN];
    __shared__ int sc[MONO_BZ][MONO_WIN];
    sa[wave][lane] = acc;
    sc[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0) {
        rows[(long)bid * MONO_WIN + lane] = ((sa[0][lane] + sa[1][lane]) + sa[2][lane]) + sa[3][lane];
        const int c = sc[0][lane] + sc[1][lane] + sc[2][lane] + sc[3][lane];
        if (c > 0 && base + lane < n1d) atomicAdd(&count[base + lane], (unsigned long long)c);
        if (lane == 0) rbase[bid] = base;
    }
}

// bin = blockIdx.x * 64 + (threadIdx.x & 63); group g = threadIdx.x >> 6 takes the rows [g * chunk, (g + 1) * chunk) in row order;
// the 16 groups are then added in group order.  out[0 .. n1d): mass, out[n1d .. 2 n1d): volume = count * vol_frac
__global__ void __launch_bounds__(MONO_WIN * MONO_FINAL_GROUPS) k_radial_final(const double* __restrict__ rows, const int* __restrict__ rbase,
                                                                              int nrows, const unsigned long long* __restrict__ count,
                                                                              int n1d, double vol_frac, double* __restrict__ out)
{
    __shared__ double sg[MONO_FINAL_GROUPS][MONO_WIN];
    const int l = threadIdx.x & (MONO_WIN - 1), g = threadIdx.x / MONO_WIN;
    const int bin = (int)blockIdx.x * MONO_WIN + l;
    const int chunk = (nrows + MONO_FINAL_GROUPS - 1) / MONO_FINAL_GROUPS;
    const int r1 = (g + 1) * chunk < nrows ? (g + 1) * chunk : nrows;
    double acc = 0.0;
    for (int r = g * chunk; r < r1; ++r) {
        const int d = bin - rbase[r];
        if (d >= 0 && d < MONO_WIN) acc += rows[(long)r * MONO_WIN + d];
    }
    sg[g][l] = acc;
    __syncthreads();
    if (g == 0 && bin < n1d) {
        double s = sg[0][l];
        for (int q = 1; q < MONO_FINAL_GROUPS; ++q) s += sg[q][l];
        out[bin] = s;
        out[n1d + bin] = (double)count[bin] * vol_frac;
    }
}

// make_radial_gravity's loop (:3170-3274) by one thread: den = mass / vol where vol > 0, the three branches around
// max_radius_all_in_domain, grav[i] = -Gconst * mass_encl / rc^2
__global__ void k_radial_gravity(const double* __restrict__ mass_vol, int n1d, double dr, double max_radius, double Gconst,
                                 double* __restrict__ grav)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double* mass = mass_vol;
    const double* vol = mass_vol + n1d;
    const double halfdr = 0.5 * dr;
    double mass_encl = 0.0;
    double vol_total_i = 0.0, vol_outer_shell = 0.0, vol_upper_shell = 0.0;
    double den_im1 = 0.0;
    for (int i = 0; i < n1d; ++i) {
        double den_i = mass[i];
        if (vol[i] > 0.0) den_i /= vol[i];
        const double rlo = ((double)i) * dr;
        const double rc = ((double)i + 0.5) * dr;
        const double rhi = ((double)i + 1.0) * dr;
        if (i == 0) {
            vol_outer_shell = (4.0 / 3.0 * M_PI) * rc * rc * rc;
            vol_upper_shell = (4.0 / 3.0 * M_PI) * (rhi * rhi * rhi - rc * rc * rc);
            vol_total_i = vol_outer_shell + vol_upper_shell;
            mass_encl = vol_outer_shell * mass[i] / vol_total_i;
        } else {
            const double vol_inner_shell = vol_upper_shell;
            const double vol_total_im1 = vol_total_i;
            vol_outer_shell = (4.0 / 3.0 * M_PI) * halfdr * (rc * rc + rlo * rc + rlo * rlo);
            vol_upper_shell = (4.0 / 3.0 * M_PI) * halfdr * (rc * rc + rhi * rc + rhi * rhi);
            vol_total_i = vol_outer_shell + vol_upper_shell;
            if (rc < max_radius)
                mass_encl = mass_encl + (vol_inner_shell / vol_total_im1) * mass[i - 1] + (vol_outer_shell / vol_total_i) * mass[i];
            else
                mass_encl = mass_encl + vol_inner_shell * den_im1 + vol_outer_shell * den_i;
        }
        grav[i] = -Gconst * mass_encl / (rc * rc);
        den_im1 = den_i;
    }
}

// interpolate_monopole_grav (:1325-1404) over [lo, lo + n) of the gravity FAB (its whole box, ghost zones included); a zone
// beyond the last bin is left as it is
__global__ void __launch_bounds__(256) k_monopole_grav(const double* __restrict__ rg, MonoGeom G, DFab F, int lo0, int lo1, int lo2,
                                                       int n0, int n1, int n2)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long)n0 * n1 * n2) return;
    const int i = lo0 + (int)(tid % n0);
    const long rr = tid / n0;
    const int j = lo1 + (int)(rr % n1), k = lo2 + (int)(rr / n1);
    const int n1d = G.n1d;
    const double dr = G.dx[0] / (double)G.drdxfac;
    double loc[3];
    loc[0] = G.problo[0] + ((double)i + 0.5) * G.dx[0] - G.center[0];
    loc[1] = G.problo[1] + ((double)j + 0.5) * G.dx[1] - G.center[1];
    loc[2] = G.problo[2] + ((double)k + 0.5) * G.dx[2] - G.center[2];
    const double r = sqrt(loc[0] * loc[0] + loc[1] * loc[1] + loc[2] * loc[2]);
    const double q = r / dr;
    if (!(q < 2.0e9)) return;
    const int index = (int)q;
    if (index > n1d - 1) return;
    const double cen = ((double)index + 0.5) * dr;
    const double xi = r - cen;
    double mag_grav;
    if (index == 0) {
        const double slope = (rg[index + 1] - rg[index]) / dr;
        mag_grav = rg[index] + slope * xi;
    } else if (index == n1d - 1) {
        const double slope = (rg[index] - rg[index - 1]) / dr;
        mag_grav = rg[index] + slope * xi;
    } else {
        const double ghi = rg[index + 1], gmd = rg[index], glo = rg[index - 1];
        mag_grav = (ghi - 2.0 * gmd + glo) * xi * xi / (2.0 * dr * dr) +
                   (ghi - glo) * xi / (2.0 * dr) +
                   (-ghi + 26.e0 * gmd - glo) / 24.e0;
        const double minvar = fmin(gmd, fmin(glo, ghi));
        const double maxvar = fmax(gmd, fmax(glo, ghi));
        mag_grav = fmax(mag_grav, minvar);
        mag_grav = fmin(mag_grav, maxvar);
    }
    const long c = (long)(i - F.lo[0]) + F.sy * (long)(j - F.lo[1]) + F.sz * (long)(k - F.lo[2]);
    for (int n = 0; n < 3; ++n) F.p[c + F.sn * n] = mag_grav * (loc[n] / r);
}

// bricks per direction and the first workgroup of every box; returns the number of workgroups or a negative error
template <class BOX>
static long mono_layout(int nbox, BOX* boxes, std::vector<int>& start)
{
    start.assign((size_t)nbox + 1, 0);
    long tot = 0;
    for (int r = 0; r < nbox; ++r) {
        BOX& B = boxes[r];
        B.nb[0] = (B.n[0] + MONO_BX - 1) / MONO_BX; B.nb[1] = (B.n[1] + MONO_BY - 1) / MONO_BY; B.nb[2] = (B.n[2] + MONO_BZ - 1) / MONO_BZ;
        if (B.n[0] > 0 && B.n[1] > 0 && B.n[2] > 0) tot += (long)B.nb[0] * B.nb[1] * B.nb[2];
        else B.nb[0] = B.nb[1] = B.nb[2] = 0;
        if (tot >= 0x3fffffffL) return CASTRO_AMD_ERR_ARG;
        start[(size_t)r + 1] = (int)tot;
    }
    return tot;
}

void mono_workspace_free(MonoWorkspace* ws)
{
    if (ws->rows) (void)hipFree(ws->rows);
    if (ws->rbase) (void)hipFree(ws->rbase);
    if (ws->count) (void)hipFree(ws->count);
    ws->tables.release();
    ws->rows = nullptr; ws->rbase = nullptr; ws->count = nullptr; ws->nrows = 0; ws->ncount = 0;
}

static void radial_partial_launch(const MonoBoxDev* tab, const int* start, int nbox, const MonoGeom& G, MonoWorkspace* ws, int nb,
                                  hipStream_t stream, Profiler* prof)
{
    prof_begin(prof, "k_radial_partial", stream);
    hipLaunchKernelGGL((k_radial_partial<false, MonoBoxDev>), dim3((unsigned)nb), dim3(MONO_WG), 0, stream, tab, start, nbox, G, ws->rows, ws->rbase, ws->count);
    prof_end(prof, stream);
}

static void radial_partial_launch(const MonoBoxDevEx* tab, const int* start, int nbox, const MonoGeom& G, MonoWorkspace* ws, int nb,
                                  hipStream_t stream, Profiler* prof)
{
    prof_begin(prof, "k_radial_partial_interp", stream);
    hipLaunchKernelGGL((k_radial_partial<true, MonoBoxDevEx>), dim3((unsigned)nb), dim3(MONO_WG), 0, stream, tab, start, nbox, G, ws->rows, ws->rbase,
                       ws->count);
    prof_end(prof, stream);
}

template <class BOX>
static int launch_radial_mass_t(int nbox, BOX* boxes, const MonoGeom& G, MonoWorkspace* ws, double* d_out, hipStream_t stream,
                                Profiler* prof)
{
    if (G.n1d < 2 || G.drdxfac < 1) return CASTRO_AMD_ERR_ARG;
    if (!radial_window_ok(G)) return CASTRO_AMD_ERR_UNSUPPORTED;
    std::vector<int> start;
    const long tot = mono_layout(nbox, boxes, start);
    if (tot < 0) return (int)tot;
    const int nb = (int)tot;
    // the workspace of the context: grown only by a call with more workgroups (or bins) than any before
    if ((size_t)nb > ws->nrows) {
        if (ws->rows) { (void)hipStreamSynchronize(stream); (void)hipFree(ws->rows); (void)hipFree(ws->rbase); ws->rows = nullptr; ws->rbase = nullptr; ws->nrows = 0; }
        if (hipMalloc(&ws->rows, (size_t)nb * MONO_WIN * sizeof(double)) != hipSuccess) return CASTRO_AMD_ERR_NOMEM;
        if (hipMalloc(&ws->rbase, (size_t)nb * sizeof(int)) != hipSuccess) return CASTRO_AMD_ERR_NOMEM;
        ws->nrows = (size_t)nb;
    }
    if ((size_t)G.n1d > ws->ncount) {
        if (ws->count) { (void)hipStreamSynchronize(stream); (void)hipFree(ws->count); ws->count = nullptr; ws->ncount = 0; }
        if (hipMalloc(&ws->count, (size_t)G.n1d * sizeof(unsigned long long)) != hipSuccess) return CASTRO_AMD_ERR_NOMEM;
        ws->ncount = (size_t)G.n1d;
    }
    // the box table on the device: kept per content (a driver alternates between the tables of its two state buffers)
    const BOX* dtab = nullptr;
    const int* dstart = nullptr;
    if (nb > 0) {
        const int rt = ws->tables.find(boxes, (size_t)nbox, start.data(), start.size(), stream, dtab, dstart);
        if (rt != 0) return rt;
    }
    if (hipMemsetAsync(ws->count, 0, (size_t)G.n1d * sizeof(unsigned long long), stream) != hipSuccess) return CASTRO_AMD_ERR_HIP;
    if (nb > 0) {
        radial_partial_launch(dtab, dstart, nbox, G, ws, nb, stream, prof);
        if (hipGetLastError() != hipSuccess) return CASTRO_AMD_ERR_HIP;
    }
    const double fac = (double)G.drdxfac;
    const double dx_frac = G.dx[0] / fac, dy_frac = G.dx[1] / fac, dz_frac = G.dx[2] / fac;
    const double vol_frac = G.octant_factor * dx_frac * dy_frac * dz_frac;
    prof_begin(prof, "k_radial_final", stream);
    hipLaunchKernelGGL(k_radial_final, dim3((unsigned)((G.n1d + MONO_WIN - 1) / MONO_WIN)), dim3(MONO_WIN * MONO_FINAL_GROUPS), 0, stream,
                       (const double*)ws->rows, (const int*)ws->rbase, nb, (const unsigned long long*)ws->count, G.n1d, vol_frac, d_out);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

int launch_radial_mass(int nbox, MonoBoxDev* boxes, const MonoGeom& G, MonoWorkspace* ws, double* d_out, hipStream_t stream,
                       Profiler* prof)
{
    return launch_radial_mass_t(nbox, boxes, G, ws, d_out, stream, prof);
}

int launch_radial_mass_ex(int nbox, MonoBoxDevEx* boxes, const MonoGeom& G, MonoWorkspace* ws, double* d_out, hipStream_t stream,
                          Profiler* prof)
{
    return launch_radial_mass_t(nbox, boxes, G, ws, d_out, stream, prof);
}

// The level combination of make_radial_gravity (Gravity.cpp:3103-3168), one thread per bin i of `level`: the level's own entry,
// then for lev = level - 1 down to 0, ratio = 2^(level - lev), the bins i < ratio * (n1d / ratio) add
// (1. / double(ratio)) * array[lev][i / ratio] -- the reference's sequence of additions to radial_mass_summed[i], and the same
// for the volumes.  out[0 .. n1d): mass, out[n1d .. 2 n1d): volume
__global__ void __launch_bounds__(256) k_radial_combine(MonoCombine A, double* __restrict__ out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int n1d = A.n1d[A.level];
    if (i >= n1d) return;
    double m = A.mv[A.level][i], v = A.mv[A.level][n1d + i];
    int ratio = 1;
    for (int lev = A.level - 1; lev >= 0; --lev) {
        ratio *= 2;
        if (i < ratio * (n1d / ratio)) {
            const double w = 1. / (double)ratio;
            const int ci = i / ratio;
            const double tm = w * A.mv[lev][ci], tv = w * A.mv[lev][A.n1d[lev] + ci];
            m += tm;
            v += tv;
        }
    }
    out[i] = m;
    out[n1d + i] = v;
}

int launch_radial_combine(const MonoCombine& A, double* d_out, hipStream_t stream, Profiler* prof)
{
    if (A.level < 0 || A.level >= MONO_MAX_LEVELS) return CASTRO_AMD_ERR_ARG;
    int ratio = 1;
    for (int lev = A.level; lev >= 0; --lev) {
        if (!A.mv[lev] || A.n1d[lev] < 2) return CASTRO_AMD_ERR_ARG;
        // the coarse index of the last bin that receives a share must exist in the coarser array
        if (lev < A.level && A.n1d[A.level] / ratio > A.n1d[lev]) return CASTRO_AMD_ERR_UNSUPPORTED;
        ratio *= 2;
    }
    const int n1d = A.n1d[A.level];
    prof_begin(prof, "k_radial_combine", stream);
    hipLaunchKernelGGL(k_radial_combine, dim3((unsigned)((n1d + 255) / 256)), dim3(256), 0, stream, A, d_out);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

// The physical-boundary fill of Gravity_Type (Castro_setup.cpp:614-622): components 0 / 1 / 2 carry the x / y / z velocity BC
// records with inflow replaced -- first-order extrapolation at inflow and outflow faces, reflection at symmetry faces and walls
// with the component normal to a mirrored face negated.  One thread per zone of [flo, flo + n); a zone inside the domain in
// every non-periodic direction is left alone.  The x, y, z sweeps of the boundary functions compose to an independent index map
// per direction (k_bc_fill of aux_kernels.hip), so every zone reads a zone inside the domain: no zone written here is read here.
struct MonoBcMap { int lo[3], hi[3]; int kind_lo[3], kind_hi[3]; };    // kind 0: leave, 1: extrapolate, 2: mirror

__global__ void __launch_bounds__(256) k_grav_bc_fill(DFab F, int lo0, int lo1, int lo2, int n0, int n1, int n2, MonoBcMap M)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long)n0 * n1 * n2) return;
    int ijk[3], s[3];
    bool flip[3], outside = false;
    ijk[0] = lo0 + (int)(tid % n0);
    const long rr = tid / n0;
    ijk[1] = lo1 + (int)(rr % n1);
    ijk[2] = lo2 + (int)(rr / n1);
    for (int d = 0; d < 3; ++d) {
        s[d] = ijk[d];
        flip[d] = false;
        if (ijk[d] < M.lo[d] && M.kind_lo[d] != 0) {
            outside = true;
            if (M.kind_lo[d] == 1) s[d] = M.lo[d];
            else { s[d] = 2 * M.lo[d] - ijk[d] - 1; flip[d] = true; }
        } else if (ijk[d] > M.hi[d] && M.kind_hi[d] != 0) {
            outside = true;
            if (M.kind_hi[d] == 1) s[d] = M.hi[d];
            else { s[d] = 2 * M.hi[d] - ijk[d] + 1; flip[d] = true; }
        }
    }
    if (!outside) return;
    const long cd = (long)(ijk[0] - F.lo[0]) + F.sy * (long)(ijk[1] - F.lo[1]) + F.sz * (long)(ijk[2] - F.lo[2]);
    const long cs = (long)(s[0] - F.lo[0]) + F.sy * (long)(s[1] - F.lo[1]) + F.sz * (long)(s[2] - F.lo[2]);
    for (int n = 0; n < 3; ++n) {
        const double v = F.p[cs + F.sn * n];
        F.p[cd + F.sn * n] = flip[n] ? -v : v;
    }
}

int launch_grav_bc_fill(const DFab& F, const int flo[3], const int fhi[3], const int domlo[3], const int domhi[3],
                        const int lo_bc[3], const int hi_bc[3], hipStream_t stream, Profiler* prof)
{
    MonoBcMap M;
    long n = 1;
    for (int d = 0; d < 3; ++d) {
        M.lo[d] = domlo[d]; M.hi[d] = domhi[d];
        M.kind_lo[d] = lo_bc[d] == 0 ? 0 : (lo_bc[d] >= 3 ? 2 : 1);      // Symmetry, SlipWall, NoSlipWall mirror
        M.kind_hi[d] = hi_bc[d] == 0 ? 0 : (hi_bc[d] >= 3 ? 2 : 1);
        if (fhi[d] < flo[d]) return 0;
        n *= fhi[d] - flo[d] + 1;
        // every zone outside the domain must find its image inside the FAB and inside the domain
        const int elo = M.kind_lo[d] != 0 && flo[d] < domlo[d] ? domlo[d] - flo[d] : 0;
        const int ehi = M.kind_hi[d] != 0 && fhi[d] > domhi[d] ? fhi[d] - domhi[d] : 0;
        if (elo > 0 && (fhi[d] < domlo[d] || (M.kind_lo[d] == 2 && domlo[d] + elo - 1 > (fhi[d] < domhi[d] ? fhi[d] : domhi[d])))) return CASTRO_AMD_ERR_ARG;
        if (ehi > 0 && (flo[d] > domhi[d] || (M.kind_hi[d] == 2 && domhi[d] - ehi + 1 < (flo[d] > domlo[d] ? flo[d] : domlo[d])))) return CASTRO_AMD_ERR_ARG;
    }
    prof_begin(prof, "k_grav_bc_fill", stream);
    hipLaunchKernelGGL(k_grav_bc_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, F, flo[0], flo[1], flo[2],
                       fhi[0] - flo[0] + 1, fhi[1] - flo[1] + 1, fhi[2] - flo[2] + 1, M);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

int launch_radial_gravity(const MonoGeom& G, const double* d_mass_vol, double* d_radial_grav, hipStream_t stream, Profiler* prof)
{
    if (G.n1d < 2 || G.drdxfac < 1) return CASTRO_AMD_ERR_ARG;
    const double dr = G.dx[0] / (double)G.drdxfac;
    prof_begin(prof, "k_radial_gravity", stream);
    hipLaunchKernelGGL(k_radial_gravity, dim3(1), dim3(64), 0, stream, d_mass_vol, G.n1d, dr, G.max_radius, G.Gconst, d_radial_grav);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

int launch_monopole_grav(const double* d_radial_grav, const MonoGeom& G, const DFab& F, const int lo[3], const int hi[3],
                         hipStream_t stream, Profiler* prof)
{
    if (G.n1d < 2 || G.drdxfac < 1) return CASTRO_AMD_ERR_ARG;
    const int n0 = hi[0] - lo[0] + 1, n1 = hi[1] - lo[1] + 1, n2 = hi[2] - lo[2] + 1;
    const long n = (long)n0 * n1 * n2;
    if (n0 <= 0 || n1 <= 0 || n2 <= 0) return 0;
    prof_begin(prof, "k_monopole_grav", stream);
    hipLaunchKernelGGL(k_monopole_grav, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_radial_grav, G, F, lo[0], lo[1], lo[2],
                       n0, n1, n2);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

} // namespace cad

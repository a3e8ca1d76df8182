// aux_kernels.hip -- per-zone passes the driver runs either side of the hydro update:
// clean_state, CFL/min-density reduction, physical-BC ghost fill, FAB copy / halo pack,
// problem initial data.  Reference locations are cited per kernel.
#include <hip/hip_runtime.h>
#include <cstring>
#include <type_traits>
#include "../../include/castro_hydro_amd.h"
#include "hydro_device.h"
#include "ctu_kernels.h"

namespace cad {
// a launch that cannot be queued (bad configuration, lost device) is reported to the caller as CASTRO_AMD_ERR_HIP
static inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP; }
}

namespace cad {

__device__ __forceinline__ long fidx(const DFab& f, int i, int j, int k, int n)
{
    return (long)(i - f.lo[0]) + f.sy * (long)(j - f.lo[1]) + f.sz * (long)(k - f.lo[2]) + f.sn * (long)n;
}

__device__ __forceinline__ bool box_thread3(const int lo[3], const int n[3], int& i, int& j, int& k)
{
    long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)n[0] * n[1] * n[2];
    if (tid >= total) return false;
    int ii = (int)(tid % n[0]);
    long r = tid / n[0];
    i = lo[0] + ii; j = lo[1] + (int)(r % n[1]); k = lo[2] + (int)(r / n[1]);
    return true;
}

struct Box3 { int lo[3]; int n[3]; };

// ---------------------------------------------------------------------------------------
// Castro::clean_state (Source/driver/Castro.cpp:4238-4278) applied `ntimes` in a row:
//   do_enforce_minimum_density  Source/hydro/advection_util.cpp:1080-1172
//   normalize_species           Source/driver/Castro.cpp:2902-2948
//   reset_internal_energy       Source/driver/Castro.cpp:3353-3414
//   computeTemp (EOS re -> T)   Source/driver/Castro.cpp:3682-3707
// Every stage is zone-local, so running the whole chain per zone is identical to the
// reference's stage-by-stage sweeps.
// ---------------------------------------------------------------------------------------
// Up to CLEAN_BOXES_MAX regions in one launch; region r owns threads [start[r], start[r+1]).  The ONE compiled copy of the plain
// clean sweep: castro_amd_clean_state_fab is a table of one region, CASTRO_AMD_OP_CLEAN of castro_amd_fab_ops_p a table of many,
// so a level cleaned box by box and one cleaned through an operation table get the same bits in the `contract` build too
// (two compiled copies of clean_zone may contract differently).
#define CLEAN_BOXES_MAX 32
struct CleanBoxes { int n; int ntimes[CLEAN_BOXES_MAX]; long start[CLEAN_BOXES_MAX + 1]; DFab U[CLEAN_BOXES_MAX]; Box3 b[CLEAN_BOXES_MAX]; };
static_assert(sizeof(CleanBoxes) + sizeof(DevParams) <= 4096, "k_clean_state: the by-value table must fit the 4 KB of kernel arguments");

__global__ void __launch_bounds__(256) k_clean_state(CleanBoxes T, DevParams P)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= T.start[T.n]) return;
    int r = 0;
    while (tid >= T.start[r + 1]) ++r;
    const DFab U = T.U[r];
    const Box3 b = T.b[r];
    const long t = tid - T.start[r];
    const int i = b.lo[0] + (int)(t % b.n[0]);
    const long rr = t / b.n[0];
    const int j = b.lo[1] + (int)(rr % b.n[1]);
    const int k = b.lo[2] + (int)(rr / b.n[1]);
    const long c = fidx(U, i, j, k, 0);
    double rho = U.p[c + U.sn * URHO];
    double mx = U.p[c + U.sn * UMX];
    double my = U.p[c + U.sn * UMY];
    double mz = U.p[c + U.sn * UMZ];
    double eden = U.p[c + U.sn * UEDEN];
    double eint = U.p[c + U.sn * UEINT];
    double temp = U.p[c + U.sn * UTEMP];
    double rX = U.p[c + U.sn * UFS];

    clean_zone(P, T.ntimes[r], rho, mx, my, mz, eden, eint, temp, rX);

    U.p[c + U.sn * URHO] = rho;
    U.p[c + U.sn * UMX] = mx;
    U.p[c + U.sn * UMY] = my;
    U.p[c + U.sn * UMZ] = mz;
    U.p[c + U.sn * UEDEN] = eden;
    U.p[c + U.sn * UEINT] = eint;
    U.p[c + U.sn * UTEMP] = temp;
    U.p[c + U.sn * UFS] = rX;
}

// clean_state x ntimes[r] on [lo + 3 r, hi + 3 r] of U[r], r < nbox: one launch per CLEAN_BOXES_MAX non-empty regions
int launch_clean_state_boxes(int nbox, const DFab* U, const int* lo, const int* hi, const int* ntimes, const DevParams& P,
                             hipStream_t stream, Profiler* prof)
{
    int done = 0;
    while (done < nbox) {
        CleanBoxes T;
        T.n = 0;
        T.start[0] = 0;
        for (; done < nbox && T.n < CLEAN_BOXES_MAX; ++done) {
            Box3 b;
            long n = 1;
            for (int d = 0; d < 3; ++d) { b.lo[d] = lo[3 * done + d]; b.n[d] = hi[3 * done + d] - lo[3 * done + d] + 1; n *= b.n[d] > 0 ? b.n[d] : 0; }
            if (n <= 0 || ntimes[done] <= 0) continue;          // nothing to clean
            T.U[T.n] = U[done]; T.b[T.n] = b; T.ntimes[T.n] = ntimes[done];
            T.start[T.n + 1] = T.start[T.n] + n;
            ++T.n;
        }
        if (T.n == 0) continue;
        prof_begin(prof, "k_clean_state", stream);
        hipLaunchKernelGGL(k_clean_state, dim3((unsigned)((T.start[T.n] + 255) / 256)), dim3(256), 0, stream, T, P);
        prof_end(prof, stream);
    }
    return launch_status();
}

int launch_clean_state(const DFab& U, const int lo[3], const int hi[3], const DevParams& P, int ntimes,
                       hipStream_t stream, Profiler* prof)
{
    return launch_clean_state_boxes(1, &U, lo, hi, &ntimes, P, stream, prof);
}

// The same sweep with the reductions of the advance: [min dx/(c+|u|) of the CLEANED state, min density of the RAW state]
// (Castro::estdt_cfl, timestep.cpp:31-140, and S_new.min(URHO), Castro_advance_ctu.cpp:168)
// through one atomic pair per block.  Grid-stride so the number of atomics stays small.
__global__ void __launch_bounds__(256) k_clean_state_reduce(DFab U, Box3 b, DevParams P, int ntimes,
                                                            double dx0, double dx1, double dx2, double* red)
{
    double dtmin = 1.e200, rmin_raw = 1.e300, dtmin1 = 1.e200;
    const long total = (long)b.n[0] * b.n[1] * b.n[2];
    for (long tid = (long)blockIdx.x * blockDim.x + threadIdx.x; tid < total; tid += (long)gridDim.x * blockDim.x) {
    const int i = b.lo[0] + (int)(tid % b.n[0]);
    const long rr = tid / b.n[0];
    const int j = b.lo[1] + (int)(rr % b.n[1]);
    const int k = b.lo[2] + (int)(rr / b.n[1]);
    const long c = fidx(U, i, j, k, 0);
    double rho = U.p[c + U.sn * URHO];
    double mx = U.p[c + U.sn * UMX];
    double my = U.p[c + U.sn * UMY];
    double mz = U.p[c + U.sn * UMZ];
    double eden = U.p[c + U.sn * UEDEN];
    double eint = U.p[c + U.sn * UEINT];
    double temp = U.p[c + U.sn * UTEMP];
    double rX = U.p[c + U.sn * UFS];
    rmin_raw = fmin(rmin_raw, nan_guard(rho));

    double d1, d2;
    clean_zone_dt(P, ntimes, dx0, dx1, dx2, rho, mx, my, mz, eden, eint, temp, rX, d1, d2);
    dtmin1 = fmin(dtmin1, d1);
    dtmin = fmin(dtmin, d2);

    U.p[c + U.sn * URHO] = rho;
    U.p[c + U.sn * UMX] = mx;
    U.p[c + U.sn * UMY] = my;
    U.p[c + U.sn * UMZ] = mz;
    U.p[c + U.sn * UEDEN] = eden;
    U.p[c + U.sn * UEINT] = eint;
    U.p[c + U.sn * UTEMP] = temp;
    U.p[c + U.sn * UFS] = rX;

    }
    block_min3_atomic(dtmin, rmin_raw, dtmin1, red);
}

int launch_clean_state_reduce(const DFab& U, const int lo[3], const int hi[3], const DevGeom& g, const DevParams& P,
                              int ntimes, double* d_out, hipStream_t stream, Profiler* prof)
{
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    long nb = (n + 255) / 256;
    if (nb > 2048) nb = 2048;            // 256 CUs x 8 blocks; grid-stride the rest
    prof_begin(prof, "k_clean_state_reduce", stream);
    hipLaunchKernelGGL(k_clean_state_reduce, dim3((unsigned)nb), dim3(256), 0, stream, U, b, P, ntimes,
                       g.dx[0], g.dx[1], g.dx[2], d_out);
    prof_end(prof, stream);
    return launch_status();
}

// ---------------------------------------------------------------------------------------
// Castro::estdt_cfl (Source/driver/timestep.cpp:31-140) + S_new.min(URHO)
// (Castro_advance_ctu.cpp:168): wave shuffle -> LDS -> one atomic per block
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_estdt(DFab U, Box3 b, double dx0, double dx1, double dx2,
                                               DevParams P, double* out)
{
    double dtmin = 1.e200, rmin = 1.e300;
    const long total = (long)b.n[0] * b.n[1] * b.n[2];
    for (long tid = (long)blockIdx.x * blockDim.x + threadIdx.x; tid < total; tid += (long)gridDim.x * blockDim.x) {
        const int i = b.lo[0] + (int)(tid % b.n[0]);
        const long rr = tid / b.n[0];
        const int j = b.lo[1] + (int)(rr % b.n[1]);
        const int k = b.lo[2] + (int)(rr / b.n[1]);
        const long c = fidx(U, i, j, k, 0);
        const double rho = U.p[c + U.sn * URHO];
        double rhoInv = 1.0 / rho;
        double e = U.p[c + U.sn * UEINT] * rhoInv;
        double p = (P.gamma - 1.0) * rho * e;
        double cs = sqrt(P.gamma * p / rho);

        double ux = U.p[c + U.sn * UMX] * rhoInv;
        double uy = U.p[c + U.sn * UMY] * rhoInv;
        double uz = U.p[c + U.sn * UMZ] * rhoInv;

        double dt1 = dx0 / (cs + fabs(ux));
        double dt2 = dx1 / (cs + fabs(uy));
        double dt3 = dx2 / (cs + fabs(uz));

        // NaNs are dropped here, like the reference's std::min fold (timestep.cpp:131-137): the consumers of this
        // estimate (estTimeStep, computeInitialDt, computeNewDt) have no retry path; they reject a non-positive or
        // non-finite result instead (castro.py / amr.py: _checked_estimate).  The guarded minima are those of the advance.
        dtmin = fmin(dtmin, amin(amin(dt1, dt2), dt3));
        rmin = fmin(rmin, rho);
    }
    block_min2_atomic(dtmin, rmin, out);
}

// ---------------------------------------------------------------------------------------
// castro_amd_step_control: the host's work between two hydro updates of a single level, by one thread
//   do_advance_ctu's checks (Castro_advance_ctu.cpp:168-216, 386-392), time += dt, Castro::computeNewDt (Castro.cpp:1629-1819)
// The expressions are those of castro.py (Castro.do_advance_ctu / computeNewDt), in the same order.
// ---------------------------------------------------------------------------------------
__global__ void k_step_control(double* red, double* ctl, double cfl, double change_max, double small_dens, double max_dt,
                               double fixed_dt, double stop_time, int retry_form)
{
    // the host's expressions in the host's order in BOTH builds: with -fassociative-math (part of the `contract` build's flags until round 6) the single
    // subcycle (time + dt) - time below was folded to dt, one ulp away from what Castro.subcycle_advance_ctu (and the
    // reference, Castro_advance_ctu.cpp:463-471) computes every now and then -- a graph-replayed batch then left the bits of
    // the stepwise driver (round 6, profiles/r06a_*)
#pragma clang fp reassociate(off) contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double est = red[0], rho_min = red[1], est1 = red[2];
    red[0] = 1.e200; red[1] = 1.e200; red[2] = 1.e200;
    if (ctl[3] != 0.0) return;                               // a rejected step: the host finds time / nstep / dt of the failure
    const double dt = ctl[0], dt_hydro = ctl[6];
    ctl[4] = rho_min; ctl[5] = est;
    int status = 0;
    if (rho_min < small_dens) status |= 1;
    const double chk = fixed_dt > 0.0 ? fixed_dt : amin(max_dt, est1 * cfl);
    if (change_max * chk < dt_hydro) status |= 2;
    if (status) { ctl[3] = (double)status; return; }
    const long n = (long)ctl[2];
    ctl[8 + (int)(n % 56)] = dt;
    const double time = ctl[1] + dt;
    ctl[1] = time;
    ctl[2] = (double)(n + 1);
    double dt_0 = fixed_dt > 0.0 ? fixed_dt : amin(max_dt, est * cfl);
    if (fixed_dt <= 0.0) dt_0 = amin(dt_0, change_max * dt);
    const double eps = 2.220446049250313e-16;
    if (stop_time >= 0.0 && (time + dt_0) >= (stop_time - eps)) dt_0 = stop_time - time;
    ctl[0] = dt_0;
    // castro.use_retry: the advance goes through subcycle_advance_ctu, whose single subcycle is (time + dt) - time
    // (Castro_advance_ctu.cpp:463-471) -- not always dt in the last bit
    ctl[6] = retry_form ? (time + dt_0) - time : dt_0;
}

int launch_step_control(double* red, double* ctl, double cfl, double change_max, double small_dens, double max_dt,
                        double fixed_dt, double stop_time, int retry_form, hipStream_t stream, Profiler* prof)
{
    prof_begin(prof, "k_step_control", stream);
    hipLaunchKernelGGL(k_step_control, dim3(1), dim3(64), 0, stream, red, ctl, cfl, change_max, small_dens, max_dt, fixed_dt, stop_time, retry_form);
    prof_end(prof, stream);
    return launch_status();
}

int launch_estdt(const DFab& U, const int lo[3], const int hi[3], const DevGeom& g, const DevParams& P,
                 double* d_out, hipStream_t stream, Profiler* prof)
{
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    long nb = (n + 255) / 256;
    if (nb > 2048) nb = 2048;
    prof_begin(prof, "k_estdt", stream);
    hipLaunchKernelGGL(k_estdt, dim3((unsigned)nb), dim3(256), 0, stream, U, b,
                       g.dx[0], g.dx[1], g.dx[2], P, d_out);
    prof_end(prof, stream);
    return launch_status();
}

// ---------------------------------------------------------------------------------------
// constant-gravity source terms (Source/gravity/Castro_gravity.cpp:234-614; gravity.gravity_type =
// "ConstantGrav": the same vector in every zone, ghost zones included, Gravity.cpp:860-866) and
// Castro::apply_source_to_state (Source/sources/Castro_sources.cpp:10-19)
// ---------------------------------------------------------------------------------------
constexpr int NSRC = 7;

// where a zone's gravity comes from: one vector for every zone (ConstantGrav), or a 3-component FAB (MonopoleGrav: gold(i,j,k,n) /
// gnew(i,j,k,n) of the reference; the grav_source_type = 4 energy term reads the six neighbours, so the FAB has one ghost zone)
struct GravConst {
    double g[3];
    __device__ __forceinline__ double operator()(int, int, int, int n) const { return g[n]; }
};
struct GravFab {
    DFab G;
    __device__ __forceinline__ double operator()(int i, int j, int k, int n) const { return G.p[fidx(G, i, j, k, n)]; }
};

// the source of one zone (src[0 .. NSRC-1], every component set); the kernels below accumulate it into the Source_Type FAB
template <class GRAV>
__device__ __forceinline__ void old_grav_zone_g(const DFab& U, int i, int j, int k, const GRAV& grav, int type, double dt, double src[7])
{
    constexpr int NSRC_ = 7;
    double snew[NUM_STATE];
    for (int n = 0; n < NSRC_; ++n) src[n] = 0.0;
    const long c = fidx(U, i, j, k, 0);
    double rho = U.p[c + U.sn * URHO];
    double rhoInv = 1.0 / rho;
    for (int n = 0; n < NUM_STATE; ++n) snew[n] = U.p[c + U.sn * n];
    const double u_mx = snew[UMX], u_my = snew[UMY], u_mz = snew[UMZ];

    double old_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoInv;

    double Sr[3];
    for (int n = 0; n < 3; ++n) {
        Sr[n] = rho * grav(i, j, k, n);
        src[UMX + n] = Sr[n];
        snew[UMX + n] += dt * src[UMX + n];
    }

    double SrE;
    if (type == 1 || type == 2) {
        SrE = (u_mx * Sr[0] + u_my * Sr[1] + u_mz * Sr[2]) * rhoInv;
    } else if (type == 3) {
        double new_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoInv;
        SrE = new_ke - old_ke;
    } else {
        SrE = (u_mx * Sr[0] + u_my * Sr[1] + u_mz * Sr[2]) * rhoInv;
    }
    src[UEDEN] = SrE;
}

__device__ __forceinline__ void old_grav_zone(const DFab& U, int i, int j, int k, const double grav[3], int type, double dt, double src[7])
{
    const GravConst g = { { grav[0], grav[1], grav[2] } };
    old_grav_zone_g(U, i, j, k, g, type, dt, src);
}

__global__ void __launch_bounds__(256) k_old_grav_source_gfab(DFab U, DFab SRC, Box3 b, GravFab gold, int type, double dt)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    double src[NSRC];
    old_grav_zone_g(U, i, j, k, gold, type, dt, src);
    const long cs = fidx(SRC, i, j, k, 0);
    for (int n = 0; n < NSRC; ++n) SRC.p[cs + SRC.sn * n] += src[n];
}

__global__ void __launch_bounds__(256) k_old_grav_source(DFab U, DFab SRC, Box3 b, double g0, double g1, double g2,
                                                         int type, double dt)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    const double grav[3] = { g0, g1, g2 };
    double src[NSRC];
    old_grav_zone(U, i, j, k, grav, type, dt, src);
    const long cs = fidx(SRC, i, j, k, 0);
    for (int n = 0; n < NSRC; ++n) SRC.p[cs + SRC.sn * n] += src[n];
}

template <class GOLD, class GNEW>
__device__ __forceinline__ void new_grav_zone_g(const DFab& UO, const DFab& UN, const DFab& M0, const DFab& M1, const DFab& M2, int i, int j, int k,
                                                const GOLD& gold, const GNEW& gnew, int type, double dt, double dx0, double dx1, double dx2,
                                                double src[7])
{
    constexpr int NSRC = 7;
    const double vol = dx0 * dx1 * dx2;
    for (int n = 0; n < NSRC; ++n) src[n] = 0.0;
    double hdtInv = 0.5 / dt;

    const long co = fidx(UO, i, j, k, 0), cn = fidx(UN, i, j, k, 0);
    double rhoo = UO.p[co + UO.sn * URHO];
    double rhooinv = 1.0 / UO.p[co + UO.sn * URHO];
    double rhon = UN.p[cn + UN.sn * URHO];
    double rhoninv = 1.0 / UN.p[cn + UN.sn * URHO];

    double snew[NUM_STATE];
    for (int n = 0; n < NUM_STATE; ++n) snew[n] = UN.p[cn + UN.sn * n];

    double old_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoninv;

    double vold[3], Sr_old[3], vnew[3], Sr_new[3];
    for (int n = 0; n < 3; ++n) vold[n] = UO.p[co + UO.sn * (UMX + n)] * rhooinv;
    for (int n = 0; n < 3; ++n) Sr_old[n] = rhoo * gold(i, j, k, n);
    double SrE_old = vold[0] * Sr_old[0] + vold[1] * Sr_old[1] + vold[2] * Sr_old[2];

    for (int n = 0; n < 3; ++n) vnew[n] = snew[UMX + n] * rhoninv;
    for (int n = 0; n < 3; ++n) Sr_new[n] = rhon * gnew(i, j, k, n);
    double SrE_new = vnew[0] * Sr_new[0] + vnew[1] * Sr_new[1] + vnew[2] * Sr_new[2];

    double Srcorr[3];
    for (int n = 0; n < 3; ++n) Srcorr[n] = 0.5 * (Sr_new[n] - Sr_old[n]);
    for (int n = 0; n < 3; ++n) {
        src[UMX + n] = Srcorr[n];
        snew[UMX + n] += dt * src[UMX + n];
    }

    double SrEcorr;
    if (type == 1) {
        SrEcorr = 0.5 * (SrE_new - SrE_old);
    } else if (type == 2) {
        for (int n = 0; n < 3; ++n) vnew[n] = snew[UMX + n] * rhoninv;
        SrE_new = vnew[0] * Sr_new[0] + vnew[1] * Sr_new[1] + vnew[2] * Sr_new[2];
        SrEcorr = 0.5 * (SrE_new - SrE_old);
    } else if (type == 3) {
        double new_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoninv;
        SrEcorr = new_ke - old_ke;
    } else {
        SrEcorr = -SrE_old;
        // time-averaged edge-centred gravity (Castro_gravity.cpp:562-574); ConstantGrav: gold == gnew == grav in every zone
        double g[3];
        for (int n = 0; n < 3; ++n) g[n] = 0.5 * (gnew(i, j, k, n) + gold(i, j, k, n));
        double gxl = 0.5 * (g[0] + 0.5 * (gnew(i - 1, j, k, 0) + gold(i - 1, j, k, 0)));
        double gxr = 0.5 * (g[0] + 0.5 * (gnew(i + 1, j, k, 0) + gold(i + 1, j, k, 0)));
        double gyl = 0.5 * (g[1] + 0.5 * (gnew(i, j - 1, k, 1) + gold(i, j - 1, k, 1)));
        double gyr = 0.5 * (g[1] + 0.5 * (gnew(i, j + 1, k, 1) + gold(i, j + 1, k, 1)));
        double gzl = 0.5 * (g[2] + 0.5 * (gnew(i, j, k - 1, 2) + gold(i, j, k - 1, 2)));
        double gzr = 0.5 * (g[2] + 0.5 * (gnew(i, j, k + 1, 2) + gold(i, j, k + 1, 2)));

        SrEcorr += hdtInv * (M0.p[fidx(M0, i, j, k, 0)] * gxl * dx0 +
                             M0.p[fidx(M0, i + 1, j, k, 0)] * gxr * dx0 +
                             M1.p[fidx(M1, i, j, k, 0)] * gyl * dx1 +
                             M1.p[fidx(M1, i, j + 1, k, 0)] * gyr * dx1 +
                             M2.p[fidx(M2, i, j, k, 0)] * gzl * dx2 +
                             M2.p[fidx(M2, i, j, k + 1, 0)] * gzr * dx2) / vol;
    }
    src[UEDEN] = SrEcorr;
}

__device__ __forceinline__ void new_grav_zone(const DFab& UO, const DFab& UN, const DFab& M0, const DFab& M1, const DFab& M2, int i, int j, int k,
                                              const double grav[3], int type, double dt, double dx0, double dx1, double dx2, double src[7])
{
    const GravConst g = { { grav[0], grav[1], grav[2] } };
    new_grav_zone_g(UO, UN, M0, M1, M2, i, j, k, g, g, type, dt, dx0, dx1, dx2, src);
}

__global__ void __launch_bounds__(256) k_new_grav_source_gfab(DFab UO, DFab UN, DFab SRC, DFab M0, DFab M1, DFab M2, Box3 b,
                                                              GravFab gold, GravFab gnew, int type, double dt,
                                                              double dx0, double dx1, double dx2)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    double src[NSRC];
    new_grav_zone_g(UO, UN, M0, M1, M2, i, j, k, gold, gnew, type, dt, dx0, dx1, dx2, src);
    const long cs = fidx(SRC, i, j, k, 0);
    for (int n = 0; n < NSRC; ++n) SRC.p[cs + SRC.sn * n] += src[n];
}

__global__ void __launch_bounds__(256) k_new_grav_source(DFab UO, DFab UN, DFab SRC, DFab M0, DFab M1, DFab M2, Box3 b,
                                                         double g0, double g1, double g2, int type, double dt,
                                                         double dx0, double dx1, double dx2)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    const double grav[3] = { g0, g1, g2 };
    double src[NSRC];
    new_grav_zone(UO, UN, M0, M1, M2, i, j, k, grav, type, dt, dx0, dx1, dx2, src);
    const long cs = fidx(SRC, i, j, k, 0);
    for (int n = 0; n < NSRC; ++n) SRC.p[cs + SRC.sn * n] += src[n];
}

__global__ void __launch_bounds__(256) k_saxpy(DFab D, DFab S, Box3 b, double a, int ncomp)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    const long cd = fidx(D, i, j, k, 0), cs = fidx(S, i, j, k, 0);
    for (int n = 0; n < ncomp; ++n) D.p[cd + D.sn * n] += a * S.p[cs + S.sn * n];
}

// dst = base + a * src on the first nsrc components (the others copied), then clean_state x ntimes, in one pass:
// MultiFab::Copy(S_new, Sborder) + apply_source_to_state + clean_state of do_advance_ctu (Castro_advance_ctu.cpp:94,
// 127-131, 262-268).  base may be dst.
__global__ void __launch_bounds__(256) k_apply_source(DFab D, DFab B, DFab S, Box3 b, double a, int nsrc, DevParams P, int ntimes)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    const long cd = fidx(D, i, j, k, 0), cb = fidx(B, i, j, k, 0), cs = fidx(S, i, j, k, 0);
    double u[NUM_STATE];
#pragma unroll
    for (int n = 0; n < NUM_STATE; ++n) {
        u[n] = B.p[cb + B.sn * n];
        if (n < nsrc) u[n] += a * S.p[cs + S.sn * n];
    }
    if (ntimes > 0) clean_zone(P, ntimes, u[URHO], u[UMX], u[UMY], u[UMZ], u[UEDEN], u[UEINT], u[UTEMP], u[UFS]);
#pragma unroll
    for (int n = 0; n < NUM_STATE; ++n) D.p[cd + D.sn * n] = u[n];
}

int launch_apply_source(const DFab& D, const DFab& B, const DFab& S, const int lo[3], const int hi[3], double a, int nsrc,
                        const DevParams& P, int ntimes, hipStream_t stream, Profiler* prof)
{
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    prof_begin(prof, "k_apply_source", stream);
    hipLaunchKernelGGL(k_apply_source, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, D, B, S, b, a, nsrc, P, ntimes);
    prof_end(prof, stream);
    return launch_status();
}

// ---------------------------------------------------------------------------------------
// rotation source terms, state_in_rotating_frame = 1 (Source/rotation/Rotation.H:10-95,
// Source/rotation/rotation_sources.cpp:9-500; math.H:9-17; position(): Castro_util.H:87-140)
// ---------------------------------------------------------------------------------------
struct RotDev {
    double omega[3], center[3];
    int include_centrifugal, include_coriolis, rot_source_type, implicit_update;
    double dx[3], problo[3], probhi[3];
    int domlo[3], domhi[3], periodic[3];
    double M[3][3];
};

__device__ __forceinline__ void cross_product(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void rot_position(const RotDev& R, int i, int j, int k, double loc[3])
{
    const int idx[3] = { i, j, k };
    for (int d = 0; d < 3; ++d) {
        double offset = R.problo[d] + 0.5 * R.dx[d];
        if (R.periodic[d]) {
            if (idx[d] < R.domlo[d]) offset += R.probhi[d] - R.problo[d];
            if (idx[d] > R.domhi[d]) offset += R.problo[d] - R.probhi[d];
        }
        loc[d] = offset + (double)idx[d] * R.dx[d];
    }
}

__device__ __forceinline__ void rotational_acceleration(const RotDev& R, const double r[3], const double v[3], bool coriolis, double Sr[3])
{
    Sr[0] = 0.0; Sr[1] = 0.0; Sr[2] = 0.0;
    const bool c1 = R.include_centrifugal == 1;
    const bool c2 = R.include_coriolis == 1 && coriolis;
    double omega_cross_v[3];
    cross_product(R.omega, v, omega_cross_v);
    if (c1) {
        double omega_cross_r[3], omega_cross_omega_cross_r[3];
        cross_product(R.omega, r, omega_cross_r);
        cross_product(R.omega, omega_cross_r, omega_cross_omega_cross_r);
        for (int d = 0; d < 3; ++d) Sr[d] -= omega_cross_omega_cross_r[d];
    }
    if (c2) {
        for (int d = 0; d < 3; ++d) Sr[d] -= 2.0 * omega_cross_v[d];
    }
}

// Castro::fill_rotational_potential (Rotation.cpp:6-39) evaluates the potential at problo + dx * (i + 1/2) - center, not at
// position()'s (problo + dx / 2) + i * dx - center: the two differ in the last bit
__device__ __forceinline__ double rot_phi_at(const RotDev& R, int i, int j, int k)
{
    const int idx[3] = { i, j, k };
    double loc[3];
    for (int d = 0; d < 3; ++d) loc[d] = R.problo[d] + R.dx[d] * ((double)idx[d] + 0.5) - R.center[d];
    double phi = 0.0;
    if (R.include_centrifugal == 1) {
        double omega_cross_r[3];
        cross_product(R.omega, loc, omega_cross_r);
        for (int d = 0; d < 3; ++d) phi -= 0.5 * omega_cross_r[d] * omega_cross_r[d];
    }
    return phi;
}

__device__ __forceinline__ void old_rot_zone(const DFab& U, int i, int j, int k, const RotDev& R, double dt, double src[NSRC])
{
    double Sr[3], snew[NUM_STATE], loc[3], v[3];
    for (int n = 0; n < NSRC; ++n) src[n] = 0.0;
    rot_position(R, i, j, k, loc);
    for (int d = 0; d < 3; ++d) loc[d] -= R.center[d];
    const long c = fidx(U, i, j, k, 0);
    double rho = U.p[c + U.sn * URHO];
    double rhoInv = 1.0 / rho;
    for (int n = 0; n < NUM_STATE; ++n) snew[n] = U.p[c + U.sn * n];
    const double umx = snew[UMX], umy = snew[UMY], umz = snew[UMZ];
    double old_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoInv;
    v[0] = umx * rhoInv;
    v[1] = umy * rhoInv;
    v[2] = umz * rhoInv;
    rotational_acceleration(R, loc, v, true, Sr);
    for (int n = 0; n < 3; ++n) Sr[n] = rho * Sr[n];
    src[UMX] = Sr[0]; src[UMY] = Sr[1]; src[UMZ] = Sr[2];
    snew[UMX] += dt * src[UMX];
    snew[UMY] += dt * src[UMY];
    snew[UMZ] += dt * src[UMZ];
    double SrE;
    if (R.rot_source_type == 3) {
        double new_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoInv;
        SrE = new_ke - old_ke;
    } else {
        SrE = umx * rhoInv * Sr[0] + umy * rhoInv * Sr[1] + umz * rhoInv * Sr[2];
    }
    src[UEDEN] += SrE;
}

__global__ void __launch_bounds__(256) k_old_rot_source(DFab U, DFab SRC, Box3 b, RotDev R, double dt)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    double src[NSRC];
    old_rot_zone(U, i, j, k, R, dt, src);
    const long cs = fidx(SRC, i, j, k, 0);
    for (int n = 0; n < NSRC; ++n) SRC.p[cs + SRC.sn * n] += src[n];
}

__device__ __forceinline__ void new_rot_zone(const DFab& UO, const DFab& UN, const DFab& M0, const DFab& M1, const DFab& M2, int i, int j, int k,
                                             const RotDev& R, double dt, double src[NSRC])
{
    const double vol = R.dx[0] * R.dx[1] * R.dx[2];
    double Sr_old[3], Sr_new[3], Srcorr[3], snew[NUM_STATE], loc[3];
    for (int n = 0; n < NSRC; ++n) src[n] = 0.0;
    rot_position(R, i, j, k, loc);
    for (int d = 0; d < 3; ++d) loc[d] -= R.center[d];
    const long co = fidx(UO, i, j, k, 0), cn = fidx(UN, i, j, k, 0);
    double rhoo = UO.p[co + UO.sn * URHO];
    double rhooinv = 1.0 / UO.p[co + UO.sn * URHO];
    double rhon = UN.p[cn + UN.sn * URHO];
    double rhoninv = 1.0 / UN.p[cn + UN.sn * URHO];
    for (int n = 0; n < NUM_STATE; ++n) snew[n] = UN.p[cn + UN.sn * n];
    const double nm[3] = { snew[UMX], snew[UMY], snew[UMZ] };
    double old_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoninv;
    double vold[3], vnew[3];
    vold[0] = UO.p[co + UO.sn * UMX] * rhooinv;
    vold[1] = UO.p[co + UO.sn * UMY] * rhooinv;
    vold[2] = UO.p[co + UO.sn * UMZ] * rhooinv;
    rotational_acceleration(R, loc, vold, true, Sr_old);
    for (int n = 0; n < 3; ++n) Sr_old[n] = rhoo * Sr_old[n];
    double SrE_old = vold[0] * Sr_old[0] + vold[1] * Sr_old[1] + vold[2] * Sr_old[2];
    vnew[0] = nm[0] * rhoninv;
    vnew[1] = nm[1] * rhoninv;
    vnew[2] = nm[2] * rhoninv;
    rotational_acceleration(R, loc, vnew, true, Sr_new);
    for (int n = 0; n < 3; ++n) Sr_new[n] = rhon * Sr_new[n];
    double SrE_new = vnew[0] * Sr_new[0] + vnew[1] * Sr_new[1] + vnew[2] * Sr_new[2];
    for (int n = 0; n < 3; ++n) Srcorr[n] = 0.5 * (Sr_new[n] - Sr_old[n]);
    if (R.implicit_update == 1) {
        double acc[3], new_mom_tmp[3], new_mom[3] = { 0.0, 0.0, 0.0 };
        rotational_acceleration(R, loc, vnew, false, acc);
        for (int n = 0; n < 3; ++n) new_mom_tmp[n] = nm[n] - 0.5 * Sr_old[n] * dt + 0.5 * rhon * acc[n] * dt;
        for (int l = 0; l < 3; ++l)
            for (int m = 0; m < 3; ++m) new_mom[l] += R.M[l][m] * new_mom_tmp[m];
        for (int n = 0; n < 3; ++n) Srcorr[n] = (new_mom[n] - nm[n]) / dt;
    }
    src[UMX] = Srcorr[0]; src[UMY] = Srcorr[1]; src[UMZ] = Srcorr[2];
    snew[UMX] += dt * src[UMX];
    snew[UMY] += dt * src[UMY];
    snew[UMZ] += dt * src[UMZ];
    double SrEcorr;
    if (R.rot_source_type == 1) {
        SrEcorr = 0.5 * (SrE_new - SrE_old);
    } else if (R.rot_source_type == 2) {
        double vn[3], acc[3];
        vn[0] = snew[UMX] * rhoninv; vn[1] = snew[UMY] * rhoninv; vn[2] = snew[UMZ] * rhoninv;
        rotational_acceleration(R, loc, vn, true, acc);
        Sr_new[0] = rhon * acc[0]; Sr_new[1] = rhon * acc[1]; Sr_new[2] = rhon * acc[2];
        double SrE_new2 = vn[0] * Sr_new[0] + vn[1] * Sr_new[1] + vn[2] * Sr_new[2];
        SrEcorr = 0.5 * (SrE_new2 - SrE_old);
    } else if (R.rot_source_type == 3) {
        double new_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoninv;
        SrEcorr = new_ke - old_ke;
    } else {
        SrEcorr = -SrE_old;
        // phi_old == phi_new: the potential of a steady rotation
        double p0 = rot_phi_at(R, i, j, k);
        double phi = 0.5 * (p0 + p0);
        double pxl = rot_phi_at(R, i - 1, j, k), pxr = rot_phi_at(R, i + 1, j, k);
        double pyl = rot_phi_at(R, i, j - 1, k), pyr = rot_phi_at(R, i, j + 1, k);
        double pzl = rot_phi_at(R, i, j, k - 1), pzr = rot_phi_at(R, i, j, k + 1);
        double phixl = 0.5 * (pxl + pxl), phixr = 0.5 * (pxr + pxr);
        double phiyl = 0.5 * (pyl + pyl), phiyr = 0.5 * (pyr + pyr);
        double phizl = 0.5 * (pzl + pzl), phizr = 0.5 * (pzr + pzr);
        SrEcorr = SrEcorr - (0.5 / dt) * ( M0.p[fidx(M0, i, j, k, 0)] * (phi - phixl) -
                                           M0.p[fidx(M0, i + 1, j, k, 0)] * (phi - phixr) +
                                           M1.p[fidx(M1, i, j, k, 0)] * (phi - phiyl) -
                                           M1.p[fidx(M1, i, j + 1, k, 0)] * (phi - phiyr) +
                                           M2.p[fidx(M2, i, j, k, 0)] * (phi - phizl) -
                                           M2.p[fidx(M2, i, j, k + 1, 0)] * (phi - phizr) ) / vol;
    }
    src[UEDEN] = SrEcorr;
}

__global__ void __launch_bounds__(256) k_new_rot_source(DFab UO, DFab UN, DFab SRC, DFab M0, DFab M1, DFab M2, Box3 b, RotDev R, double dt)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    double src[NSRC];
    new_rot_zone(UO, UN, M0, M1, M2, i, j, k, R, dt, src);
    const long cs = fidx(SRC, i, j, k, 0);
    for (int n = 0; n < NSRC; ++n) SRC.p[cs + SRC.sn * n] += src[n];
}

// ---------------------------------------------------------------------------------------
// the sponge (castro.do_sponge, Source/sources/Castro_sponge.cpp:55-249): momentum is damped towards rho * target velocity where
// the radius, the density or the pressure of a zone says so; a new-time source only (construct_old_sponge_source is empty)
// ---------------------------------------------------------------------------------------
struct SpongeDev {
    double lower_radius, upper_radius, lower_density, upper_density, lower_pressure, upper_pressure;
    double lower_factor, upper_factor, target[3], alpha;
    double center[3], problo[3], dx[3];
    int implicit;
};

// lower_factor + 0.5 (upper_factor - lower_factor) (1 - cos(pi (x - lo) / delta)); lo == hi at x == lo is cos(pi 0/0), as in the reference
__device__ __forceinline__ double sponge_ramp(const SpongeDev& S, double x, double lo, double delta)
{
    return S.lower_factor + 0.5 * (S.upper_factor - S.lower_factor) * (1.0 - cos(M_PI * (x - lo) / delta));
}

// the sponge source of one zone from its NEW state (rho, momenta, T, rho X): Sr[3] for UMX..UMZ and SrE for UEDEN, the
// only components the sponge has
__device__ __forceinline__ void sponge_zone(const SpongeDev& S, const DevParams& P, int i, int j, int k, double rho, const double mom[3],
                                            double T, double rhoX, double dt, double Sr[3], double& SrE)
{
    const int idx[3] = { i, j, k };
    double r[3];
    for (int d = 0; d < 3; ++d) r[d] = S.problo[d] + ((double)idx[d] + 0.5) * S.dx[d] - S.center[d];
    const double rhoInv = 1.0 / rho;
    const double delta_r = S.upper_radius - S.lower_radius;
    const double delta_rho = S.lower_density - S.upper_density;
    const double delta_p = S.lower_pressure - S.upper_pressure;
    double f = 0.0;
    if (S.lower_radius >= 0.0 && S.upper_radius > S.lower_radius) {
        const double rad = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (rad < S.lower_radius) f = S.lower_factor;
        else if (rad >= S.lower_radius && rad <= S.upper_radius) f = sponge_ramp(S, rad, S.lower_radius, delta_r);
        else f = S.upper_factor;
    }
    // the density sponge takes priority over the radial one, the pressure sponge over both
    if (S.upper_density > 0.0 && S.lower_density > 0.0) {
        if (rho > S.upper_density) f = S.lower_factor;
        else if (rho <= S.upper_density && rho >= S.lower_density) f = sponge_ramp(S, rho, S.upper_density, delta_rho);
        else f = S.upper_factor;
    }
    if (S.upper_pressure > 0.0 && S.lower_pressure >= 0.0) {
        const double e = eos_e_of_T(P, T, rhoX * rhoInv);               // eos(eos_input_rt) of (rho, T, X)
        const double p = (P.gamma - 1.0) * rho * e;
        if (p > S.upper_pressure) f = S.lower_factor;
        else if (p <= S.upper_pressure && p >= S.lower_pressure) f = sponge_ramp(S, p, S.upper_pressure, delta_p);
        else f = S.upper_factor;
    }
    double fac;
    if (S.implicit == 1) fac = -(1.0 - 1.0 / (1.0 + S.alpha * f));
    else fac = -S.alpha * f;
    for (int n = 0; n < 3; ++n) Sr[n] = (mom[n] - rho * S.target[n]) * fac / dt;
    SrE = 0.0;
    for (int n = 0; n < 3; ++n) SrE += mom[n] * rhoInv * Sr[n];
}

__global__ void __launch_bounds__(256) k_new_sponge_source(DFab UN, DFab SRC, Box3 b, SpongeDev S, DevParams P, double dt)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    const long c = fidx(UN, i, j, k, 0);
    const double mom[3] = { UN.p[c + UN.sn * UMX], UN.p[c + UN.sn * UMY], UN.p[c + UN.sn * UMZ] };
    double Sr[3], SrE;
    sponge_zone(S, P, i, j, k, UN.p[c + UN.sn * URHO], mom, UN.p[c + UN.sn * UTEMP], UN.p[c + UN.sn * UFS], dt, Sr, SrE);
    const long cs = fidx(SRC, i, j, k, 0);
    for (int n = 0; n < 3; ++n) SRC.p[cs + SRC.sn * (UMX + n)] += Sr[n];
    SRC.p[cs + SRC.sn * UEDEN] += SrE;
}


static Box3 make_box3(const int lo[3], const int hi[3], long& n)
{
    Box3 b;
    n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    return b;
}

int launch_old_grav_source(const DFab& U, const DFab& SRC, const int lo[3], const int hi[3], const double grav[3],
                           int type, double dt, hipStream_t stream, Profiler* prof)
{
    long n; Box3 b = make_box3(lo, hi, n);
    if (n <= 0) return 0;
    prof_begin(prof, "k_old_grav_source", stream);
    hipLaunchKernelGGL(k_old_grav_source, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, U, SRC, b,
                       grav[0], grav[1], grav[2], type, dt);
    prof_end(prof, stream);
    return launch_status();
}

int launch_old_grav_source_gfab(const DFab& U, const DFab& SRC, const int lo[3], const int hi[3], const DFab& GO,
                                int type, double dt, hipStream_t stream, Profiler* prof)
{
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    const GravFab gold = { GO };
    prof_begin(prof, "k_old_grav_source_gfab", stream);
    hipLaunchKernelGGL(k_old_grav_source_gfab, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, U, SRC, b, gold, type, dt);
    prof_end(prof, stream);
    return launch_status();
}

int launch_new_grav_source_gfab(const DFab& UO, const DFab& UN, const DFab& SRC, const DFab M[3], const int lo[3], const int hi[3],
                                const DFab& GO, const DFab& GN, int type, double dt, const double dx[3], hipStream_t stream,
                                Profiler* prof)
{
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    const GravFab gold = { GO }, gnew = { GN };
    prof_begin(prof, "k_new_grav_source_gfab", stream);
    hipLaunchKernelGGL(k_new_grav_source_gfab, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, UO, UN, SRC, M[0], M[1], M[2], b,
                       gold, gnew, type, dt, dx[0], dx[1], dx[2]);
    prof_end(prof, stream);
    return launch_status();
}

int launch_new_grav_source(const DFab& UO, const DFab& UN, const DFab& SRC, const DFab M[3], const int lo[3], const int hi[3],
                           const double grav[3], int type, double dt, const double dx[3], hipStream_t stream, Profiler* prof)
{
    long n; Box3 b = make_box3(lo, hi, n);
    if (n <= 0) return 0;
    prof_begin(prof, "k_new_grav_source", stream);
    hipLaunchKernelGGL(k_new_grav_source, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, UO, UN, SRC, M[0], M[1], M[2], b,
                       grav[0], grav[1], grav[2], type, dt, dx[0], dx[1], dx[2]);
    prof_end(prof, stream);
    return launch_status();
}

static RotDev make_rotdev(const castro_amd_rotation* r, const castro_amd_geom* g, double dt)
{
    RotDev R;
    for (int d = 0; d < 3; ++d) {
        R.omega[d] = r->omega[d]; R.center[d] = r->center[d];
        R.dx[d] = g->dx[d]; R.problo[d] = g->problo[d]; R.probhi[d] = g->probhi[d];
        R.domlo[d] = g->domlo[d]; R.domhi[d] = g->domhi[d];
        R.periodic[d] = (g->lo_bc[d] == 0 && g->hi_bc[d] == 0) ? 1 : 0;
    }
    R.include_centrifugal = r->include_centrifugal; R.include_coriolis = r->include_coriolis;
    R.rot_source_type = r->rot_source_type; R.implicit_update = r->implicit_rotation_update;
    // the matrix of the implicit Coriolis update, rotation_sources.cpp:186-237 (host side, like the reference)
    double w[3];
    for (int d = 0; d < 3; ++d) w[d] = (r->include_coriolis == 1) ? dt * r->omega[d] : 0.0;
    for (int l = 0; l < 3; ++l) for (int m = 0; m < 3; ++m) R.M[l][m] = 0.0;
    if (r->implicit_rotation_update == 1) {
        R.M[0][0] = 1.0 + w[0] * w[0];
        R.M[0][1] = w[0] * w[1] + w[2];
        R.M[0][2] = w[0] * w[2] - w[1];
        R.M[1][0] = w[1] * w[0] - w[2];
        R.M[1][1] = 1.0 + w[1] * w[1];
        R.M[1][2] = w[1] * w[2] + w[0];
        R.M[2][0] = w[2] * w[0] + w[1];
        R.M[2][1] = w[2] * w[1] - w[0];
        R.M[2][2] = 1.0 + w[2] * w[2];
        for (int l = 0; l < 3; ++l)
            for (int m = 0; m < 3; ++m) R.M[l][m] /= (1.0 + w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    }
    return R;
}

int launch_old_rot_source(const DFab& U, const DFab& SRC, const int lo[3], const int hi[3], const castro_amd_rotation* r,
                          const castro_amd_geom* g, double dt, hipStream_t stream, Profiler* prof)
{
    long n; Box3 b = make_box3(lo, hi, n);
    if (n <= 0) return 0;
    prof_begin(prof, "k_old_rot_source", stream);
    hipLaunchKernelGGL(k_old_rot_source, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, U, SRC, b, make_rotdev(r, g, dt), dt);
    prof_end(prof, stream);
    return launch_status();
}

int launch_new_rot_source(const DFab& UO, const DFab& UN, const DFab& SRC, const DFab M[3], const int lo[3], const int hi[3],
                          const castro_amd_rotation* r, const castro_amd_geom* g, double dt, hipStream_t stream, Profiler* prof)
{
    long n; Box3 b = make_box3(lo, hi, n);
    if (n <= 0) return 0;
    prof_begin(prof, "k_new_rot_source", stream);
    hipLaunchKernelGGL(k_new_rot_source, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, UO, UN, SRC, M[0], M[1], M[2], b,
                       make_rotdev(r, g, dt), dt);
    prof_end(prof, stream);
    return launch_status();
}

static SpongeDev make_spongedev(const castro_amd_sponge* s, const castro_amd_geom* g, double dt)
{
    SpongeDev S;
    S.lower_radius = s->lower_radius; S.upper_radius = s->upper_radius;
    S.lower_density = s->lower_density; S.upper_density = s->upper_density;
    S.lower_pressure = s->lower_pressure; S.upper_pressure = s->upper_pressure;
    S.lower_factor = s->lower_factor; S.upper_factor = s->upper_factor;
    // alpha = dt / sponge_timescale (Castro_sponge.cpp:64-69), the same in every zone
    S.alpha = s->timescale > 0.0 ? dt / s->timescale : 0.0;
    for (int d = 0; d < 3; ++d) {
        S.target[d] = s->target_velocity[d]; S.center[d] = s->center[d];
        S.problo[d] = g->problo[d]; S.dx[d] = g->dx[d];
    }
    S.implicit = s->implicit;
    return S;
}

int launch_new_sponge_source(const DFab& UN, const DFab& SRC, const int lo[3], const int hi[3], const castro_amd_sponge* s,
                             const castro_amd_geom* g, const DevParams& P, double dt, hipStream_t stream, Profiler* prof)
{
    long n; Box3 b = make_box3(lo, hi, n);
    if (n <= 0) return 0;
    prof_begin(prof, "k_new_sponge_source", stream);
    hipLaunchKernelGGL(k_new_sponge_source, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, UN, SRC, b, make_spongedev(s, g, dt), P, dt);
    prof_end(prof, stream);
    return launch_status();
}

// ---------------------------------------------------------------------------------------
// castro_amd_sources_mf (round 6): a source stage of do_advance_ctu for every box of a level in ONE launch.  Per zone of the
// Source_Type FAB of its box a thread does what memset + k_old/new_grav_source + k_old/new_rot_source + k_apply_source did in
// three to four launches per box: outside the valid zones the source is zeroed; inside, the gravity and the rotation source
// are formed by the zone functions of those kernels, added to a zero in their order, stored, and applied to the state
// (base + dt * source, clean_state x ntimes) -- the same operations on the same values, hence the same bits.
// ---------------------------------------------------------------------------------------
struct GravDev { double g[3]; int type, on; };

// the SrcBoxDev of a table entry: the entry itself, or the front of an entry that carries its gravity FABs as well
__device__ __forceinline__ const SrcBoxDev& src_box_of(const SrcBoxDev& b) { return b; }
__device__ __forceinline__ const SrcBoxDev& src_box_of(const SrcBoxGDev& b) { return b.box; }

// GFAB = false (BOX = SrcBoxDev): the one vector of the call through GravConst.  GFAB = true (BOX = SrcBoxGDev,
// castro_amd_sources_mf_g): the gravity of a zone through GravFab from the box's grav_old / grav_new FABs, the zone functions
// of k_old_grav_source_gfab / k_new_grav_source_gfab
// SP: nothing, or one SpongeDev (STAGE 1 and 2) -- the sponge after rotation, sponge_zone on the S_new values this thread loads for
// the apply anyway.  Without it the kernel has the arguments and the code it had before there was a sponge.
// STAGE 2 (the source re-evaluation after a reflux, Castro.cpp:2773-2868): in front of stage 1 the zone's stored new-time source
// is taken out of S_new and the zone cleaned (k_apply_source with a = -dt), in the same thread.  The new-time zone functions read
// S_new in their own zone only -- the value this thread has just stored -- and neighbours enter through the gravity FABs and the
// face mass fluxes, which this kernel does not write: the three sweeps of the separate calls become one.
__device__ __forceinline__ const SpongeDev& sponge_arg(const SpongeDev& s) { return s; }

template <int STAGE, bool GFAB, class BOX, class... SP>
__global__ void __launch_bounds__(256) k_sources_apply(const BOX* __restrict__ tab, const long* __restrict__ start, int nbox,
                                                       GravDev G, RotDev R, int rot_on, double dt, double dx0, double dx1, double dx2,
                                                       DevParams P, int ntimes, int diff_on, SP... sp)
{
    constexpr bool SPONGE = sizeof...(SP) == 1;
    static_assert(STAGE >= 0 && STAGE <= 2, "stage 0: old time, 1: new time, 2: new time again after a reflux");
    static_assert(sizeof...(SP) <= 1 && (!SPONGE || STAGE >= 1), "the sponge is one argument of the new-time stages");
    long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= start[nbox]) return;
    int lo_ = 0, hi_ = nbox - 1;
    while (lo_ < hi_) {
        const int mid = (lo_ + hi_ + 1) >> 1;
        if (start[mid] <= t) lo_ = mid; else hi_ = mid - 1;
    }
    const BOX BX = tab[lo_];
    const SrcBoxDev& B = src_box_of(BX);
    t -= start[lo_];
    const int i = B.lo[0] + (int)(t % B.n[0]);
    const long q = t / B.n[0];
    const int j = B.lo[1] + (int)(q % B.n[1]), k = B.lo[2] + (int)(q / B.n[1]);
    const long cs = fidx(B.Src, i, j, k, 0);
    if (i < B.vlo[0] || i > B.vhi[0] || j < B.vlo[1] || j > B.vhi[1] || k < B.vlo[2] || k > B.vhi[2]) {
        for (int n = 0; n < B.nsc; ++n) B.Src.p[cs + B.Src.sn * n] = 0.0;         // the memset of the ghost zones
        return;
    }
    if constexpr (STAGE == 2) {
        // apply_source_to_state(S_new, source, -dt) and clean_state (Castro.cpp:2794-2799): k_apply_source with base == dst
        const long cn = fidx(B.Sn, i, j, k, 0);
        const double a = -dt;
        double v[NUM_STATE];
#pragma unroll
        for (int n = 0; n < NUM_STATE; ++n) {
            v[n] = B.Sn.p[cn + B.Sn.sn * n];
            if (n < NSRC) v[n] += a * B.Src.p[cs + B.Src.sn * n];
        }
        if (ntimes > 0) clean_zone(P, ntimes, v[URHO], v[UMX], v[UMY], v[UMZ], v[UEDEN], v[UEINT], v[UTEMP], v[UFS]);
#pragma unroll
        for (int n = 0; n < NUM_STATE; ++n) B.Sn.p[cn + B.Sn.sn * n] = v[n];
    }
    double acc[NSRC], src[NSRC];
    for (int n = 0; n < NSRC; ++n) acc[n] = 0.0;
    if (diff_on) {
        // diff_src comes first in the dispatch order of the sources (Castro_sources.cpp): k_temp_diffusion has left
        // 0 + the diffusion term in the two energy components of the valid zones, the other sources are added to it
        acc[UEDEN] = B.Src.p[cs + B.Src.sn * UEDEN];
        acc[UEINT] = B.Src.p[cs + B.Src.sn * UEINT];
    }
    if (G.on) {
        if constexpr (GFAB) {
            const GravFab gold = { BX.GO }, gnew = { BX.GN };
            if (STAGE == 0) old_grav_zone_g(B.So, i, j, k, gold, G.type, dt, src);
            else new_grav_zone_g(B.So, B.Sn, B.M0, B.M1, B.M2, i, j, k, gold, gnew, G.type, dt, dx0, dx1, dx2, src);
        } else {
            if (STAGE == 0) old_grav_zone(B.So, i, j, k, G.g, G.type, dt, src);
            else new_grav_zone(B.So, B.Sn, B.M0, B.M1, B.M2, i, j, k, G.g, G.type, dt, dx0, dx1, dx2, src);
        }
        for (int n = 0; n < NSRC; ++n) acc[n] += src[n];
    }
    if (rot_on) {
        if (STAGE == 0) old_rot_zone(B.So, i, j, k, R, dt, src);
        else new_rot_zone(B.So, B.Sn, B.M0, B.M1, B.M2, i, j, k, R, dt, src);
        for (int n = 0; n < NSRC; ++n) acc[n] += src[n];
    }
    double u[NUM_STATE];
    if constexpr (SPONGE) {
        // the base of the apply is S_new, the state the sponge is made from: loaded once, in front of the store of the source
        const long cn = fidx(B.Sn, i, j, k, 0);
#pragma unroll
        for (int n = 0; n < NUM_STATE; ++n) u[n] = B.Sn.p[cn + B.Sn.sn * n];
        const double mom[3] = { u[UMX], u[UMY], u[UMZ] };
        double Sr[3], SrE;
        sponge_zone(sponge_arg(sp...), P, i, j, k, u[URHO], mom, u[UTEMP], u[UFS], dt, Sr, SrE);
        for (int n = 0; n < 3; ++n) acc[UMX + n] += Sr[n];
        acc[UEDEN] += SrE;
    }
    for (int n = 0; n < B.nsc; ++n) B.Src.p[cs + B.Src.sn * n] = n < NSRC ? acc[n] : 0.0;
    // k_apply_source: S_new = (S_old | S_new) + dt * source, clean_state x ntimes
    const DFab& Bs = STAGE == 0 ? B.So : B.Sn;
    const long cd = fidx(B.Sn, i, j, k, 0), cb = fidx(Bs, i, j, k, 0);
#pragma unroll
    for (int n = 0; n < NUM_STATE; ++n) {
        if constexpr (!SPONGE) u[n] = Bs.p[cb + Bs.sn * n];
        if (n < NSRC) u[n] += dt * acc[n];
    }
    if (ntimes > 0) clean_zone(P, ntimes, u[URHO], u[UMX], u[UMY], u[UMZ], u[UEDEN], u[UEINT], u[UTEMP], u[UFS]);
#pragma unroll
    for (int n = 0; n < NUM_STATE; ++n) B.Sn.p[cd + B.Sn.sn * n] = u[n];
}

static RotDev make_rotdev(const castro_amd_rotation* r, const castro_amd_geom* g, double dt);

static const SrcBoxDev& src_box_host(const SrcBoxDev& b) { return b; }
static const SrcBoxDev& src_box_host(const SrcBoxGDev& b) { return b.box; }

template <class BOX>
static int launch_sources_apply_t(int stage, int nbox, const BOX* boxes, const double* grav, int grav_type, const castro_amd_rotation* rot,
                                  const castro_amd_geom* geom, const DevParams& P, double dt, int ntimes, StagedTable* arena,
                                  hipStream_t stream, Profiler* prof, int diff_on, const castro_amd_sponge* sponge)
{
    constexpr bool GFAB = std::is_same<BOX, SrcBoxGDev>::value;
    if (nbox < 1 || !boxes || !arena) return 0;
    std::vector<long> start((size_t)nbox + 1, 0);
    for (int r = 0; r < nbox; ++r) {
        long n = 1;
        for (int d = 0; d < 3; ++d) n *= src_box_host(boxes[r]).n[d] > 0 ? src_box_host(boxes[r]).n[d] : 0;
        start[(size_t)r + 1] = start[(size_t)r] + n;
    }
    if (start.back() <= 0) return 0;
    const BOX* dbox;
    const long* dstart;
    const int rt = arena->stage(boxes, (size_t)nbox, start.data(), start.size(), stream, dbox, dstart);
    if (rt != 0) return rt;
    GravDev G;
    G.on = (grav || GFAB) ? 1 : 0; G.type = grav_type;
    for (int d = 0; d < 3; ++d) G.g[d] = grav ? grav[d] : 0.0;
    RotDev R;
    std::memset(&R, 0, sizeof(R));
    if (rot) R = make_rotdev(rot, geom, dt);
    const unsigned nb = (unsigned)((start.back() + 255) / 256);
    // the sponge has no old-time source: stage 0 with a sponge is the launch without one
    const bool sp = sponge && stage >= 1;
    prof_begin(prof, stage == 2 ? (sp ? "k_sources_renew_sponge" : "k_sources_renew")
                                : sp ? "k_sources_new_sponge" : stage == 0 ? "k_sources_old" : "k_sources_new", stream);
    auto launch = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, stream, dbox, dstart, nbox, G, R, rot ? 1 : 0, dt, geom->dx[0], geom->dx[1],
                           geom->dx[2], P, ntimes, diff_on, tail...);
    };
    if (stage == 2 && sp) launch(k_sources_apply<2, GFAB, BOX, SpongeDev>, make_spongedev(sponge, geom, dt));
    else if (stage == 2) launch(k_sources_apply<2, GFAB, BOX>);
    else if (sp) launch(k_sources_apply<1, GFAB, BOX, SpongeDev>, make_spongedev(sponge, geom, dt));
    else if (stage == 0) launch(k_sources_apply<0, GFAB, BOX>);
    else launch(k_sources_apply<1, GFAB, BOX>);
    prof_end(prof, stream);
    return launch_status();
}

int launch_sources_apply(int stage, int nbox, const SrcBoxDev* boxes, const double* grav, int grav_type, const castro_amd_rotation* rot,
                         const castro_amd_geom* geom, const DevParams& P, double dt, int ntimes, StagedTable* arena,
                         hipStream_t stream, Profiler* prof, int diff_on, const castro_amd_sponge* sponge)
{
    return launch_sources_apply_t(stage, nbox, boxes, grav, grav_type, rot, geom, P, dt, ntimes, arena, stream, prof, diff_on, sponge);
}

int launch_sources_apply_gfab(int stage, int nbox, const SrcBoxGDev* boxes, int grav_type, const castro_amd_rotation* rot,
                              const castro_amd_geom* geom, const DevParams& P, double dt, int ntimes, StagedTable* arena,
                              hipStream_t stream, Profiler* prof, int diff_on, const castro_amd_sponge* sponge)
{
    return launch_sources_apply_t(stage, nbox, boxes, nullptr, grav_type, rot, geom, P, dt, ntimes, arena, stream, prof, diff_on, sponge);
}

int launch_saxpy(const DFab& D, const DFab& S, const int lo[3], const int hi[3], double a, int ncomp,
                 hipStream_t stream, Profiler* prof)
{
    long n; Box3 b = make_box3(lo, hi, n);
    if (n <= 0) return 0;
    prof_begin(prof, "k_saxpy", stream);
    hipLaunchKernelGGL(k_saxpy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, D, S, b, a, ncomp);
    prof_end(prof, stream);
    return launch_status();
}

// ---------------------------------------------------------------------------------------
// two-level AMR building blocks, refinement ratio 2 (FillPatch with cell_cons_interp, Castro_setup.cpp:352-364;
// FluxRegCrseInit / FluxRegFineAdd, Castro.cpp:2487-2545; reflux :2549-2700; avgDown :3096-3113).  The arithmetic
// is AMReX's (CellConservativeLinear, FluxRegister, average_down) [3P], restated; see include/castro_hydro_amd.h.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double mc_slope(double um, double u0, double up)
{
    double dl = u0 - um, dr = up - u0;
    double dc = 0.5 * (up - um);
    if (dl * dr <= 0.0) return 0.0;
    double lim = 2.0 * amin(fabs(dl), fabs(dr));
    return copysign(1.0, dc) * amin(fabs(dc), lim);
}

__device__ __forceinline__ int coarsen2(int i) { return (i >= 0) ? i / 2 : -((-i + 1) / 2); }

// cell_cons_interp of component n of the coarse FAB at fine zone (i, j, k)
__device__ __forceinline__ double cc_interp_value(const DFab& C, int i, int j, int k, int n)
{
    const int ic = coarsen2(i), jc = coarsen2(j), kc = coarsen2(k);
    const double ox = (i - 2 * ic == 0) ? -0.25 : 0.25;
    const double oy = (j - 2 * jc == 0) ? -0.25 : 0.25;
    const double oz = (k - 2 * kc == 0) ? -0.25 : 0.25;
#define CC(ii, jj, kk) C.p[fidx(C, ic + (ii), jc + (jj), kc + (kk), n)]
    const double u0 = CC(0, 0, 0);
    double sx = mc_slope(CC(-1, 0, 0), u0, CC(1, 0, 0));
    double sy = mc_slope(CC(0, -1, 0), u0, CC(0, 1, 0));
    double sz = mc_slope(CC(0, 0, -1), u0, CC(0, 0, 1));
    double umax = u0, umin = u0;
    for (int kk = -1; kk <= 1; ++kk)
    for (int jj = -1; jj <= 1; ++jj)
    for (int ii = -1; ii <= 1; ++ii) {
        double v = CC(ii, jj, kk);
        umax = amax(umax, v);
        umin = amin(umin, v);
    }
#undef CC
    const double dmax = 0.25 * (fabs(sx) + fabs(sy) + fabs(sz));
    double alpha = 1.0;
    if (dmax > umax - u0) alpha = amin(alpha, (umax - u0) / dmax);
    if (dmax > u0 - umin) alpha = amin(alpha, (u0 - umin) / dmax);
    return u0 + alpha * (sx * ox + sy * oy + sz * oz);
}

__global__ void __launch_bounds__(256) k_cc_interp(DFab C, DFab F, Box3 b, int ncomp)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    for (int n = 0; n < ncomp; ++n) F.p[fidx(F, i, j, k, n)] = cc_interp_value(C, i, j, k, n);
}

// The coarse-level part of a fine box's FillPatch in one launch: every zone of grow(valid, ng) \ valid gets the
// cell-conservative interpolation of the coarse state and then clean_state x ntimes (Castro_advance.cpp:186 cleans
// the ghost zones of Sborder too).  The shell is six slabs (z slabs over the full x-y extent, then y, then x).
__global__ void __launch_bounds__(256) k_fillpatch_shell(DFab C, DFab F, Slabs S, DevParams P, int ntimes)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= S.start[6]) return;
    int r = 0;
    while (tid >= S.start[r + 1]) ++r;
    const long t = tid - S.start[r];
    const int n0 = S.nn[r][0], n1 = S.nn[r][1];
    const int i = S.lo[r][0] + (int)(t % n0);
    const long q = t / n0;
    const int j = S.lo[r][1] + (int)(q % n1), k = S.lo[r][2] + (int)(q / n1);
    double u[NUM_STATE];
    for (int n = 0; n < NUM_STATE; ++n) u[n] = cc_interp_value(C, i, j, k, n);
    if (ntimes > 0) clean_zone(P, ntimes, u[URHO], u[UMX], u[UMY], u[UMZ], u[UEDEN], u[UEINT], u[UTEMP], u[UFS]);
    for (int n = 0; n < NUM_STATE; ++n) F.p[fidx(F, i, j, k, n)] = u[n];
}

int launch_fillpatch_shell(const DFab& C, const DFab& F, const int vlo[3], const int vhi[3], int ng, const DevParams& P, int ntimes,
                           hipStream_t stream, Profiler* prof)
{
    Slabs S;
    int glo[3], ghi[3];
    for (int d = 0; d < 3; ++d) { glo[d] = vlo[d] - ng; ghi[d] = vhi[d] + ng; }
    const int lo[6][3] = { { glo[0], glo[1], glo[2] }, { glo[0], glo[1], vhi[2] + 1 }, { glo[0], glo[1], vlo[2] },
                           { glo[0], vhi[1] + 1, vlo[2] }, { glo[0], vlo[1], vlo[2] }, { vhi[0] + 1, vlo[1], vlo[2] } };
    const int hi[6][3] = { { ghi[0], ghi[1], vlo[2] - 1 }, { ghi[0], ghi[1], ghi[2] }, { ghi[0], vlo[1] - 1, vhi[2] },
                           { ghi[0], ghi[1], vhi[2] }, { vlo[0] - 1, vhi[1], vhi[2] }, { ghi[0], vhi[1], vhi[2] } };
    S.start[0] = 0;
    for (int r = 0; r < 6; ++r) {
        long n = 1;
        for (int d = 0; d < 3; ++d) { S.lo[r][d] = lo[r][d]; S.nn[r][d] = hi[r][d] - lo[r][d] + 1; n *= S.nn[r][d] > 0 ? S.nn[r][d] : 0; }
        S.start[r + 1] = S.start[r] + n;
    }
    if (S.start[6] <= 0) return 0;
    prof_begin(prof, "k_fillpatch_shell", stream);
    hipLaunchKernelGGL(k_fillpatch_shell, dim3((unsigned)((S.start[6] + 255) / 256)), dim3(256), 0, stream, C, F, S, P, ntimes);
    prof_end(prof, stream);
    return launch_status();
}

__global__ void __launch_bounds__(256) k_avgdown(DFab F, DFab C, Box3 b, int ncomp)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    for (int n = 0; n < ncomp; ++n) {
        double s = 0.0;
        for (int kk = 0; kk < 2; ++kk)
        for (int jj = 0; jj < 2; ++jj)
        for (int ii = 0; ii < 2; ++ii) s += F.p[fidx(F, 2 * i + ii, 2 * j + jj, 2 * k + kk, n)];
        C.p[fidx(C, i, j, k, n)] = 0.125 * s;
    }
}

// mode 0: reg = mult * cflux (CrseInit); mode 1: reg += mult * sum of the 4 fine faces (FineAdd)
__global__ void __launch_bounds__(256) k_fluxreg(DFab R, DFab X, Box3 b, int dir, int ncomp, double mult, int mode)
{
    int c[3];
    if (!box_thread3(b.lo, b.n, c[0], c[1], c[2])) return;
    const int t1 = (dir + 1) % 3, t2 = (dir + 2) % 3;
    for (int n = 0; n < ncomp; ++n) {
        const long cr = fidx(R, c[0], c[1], c[2], n);
        if (mode == 0) {
            R.p[cr] = mult * X.p[fidx(X, c[0], c[1], c[2], n)];
        } else {
            int f[3];
            double s = 0.0;
            for (int bb = 0; bb < 2; ++bb)
            for (int aa = 0; aa < 2; ++aa) {
                f[dir] = 2 * c[dir];
                f[t1] = 2 * c[t1] + aa;
                f[t2] = 2 * c[t2] + bb;
                s += X.p[fidx(X, f[0], f[1], f[2], n)];
            }
            R.p[cr] += mult * s;
        }
    }
}

// flux += reg on the faces of the region, and mass_flux = flux(URHO) there where a mass-flux FAB is given: the coarse fluxes
// after a reflux (Castro.cpp:2617-2644)
__global__ void __launch_bounds__(256) k_fluxreg_to_flux(DFab F, DFab R, DFab M, Box3 b, int ncomp)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    for (int n = 0; n < ncomp; ++n) {
        const long cf = fidx(F, i, j, k, n);
        const double f = F.p[cf] + R.p[fidx(R, i, j, k, n)];
        F.p[cf] = f;
        if (n == URHO && M.p) M.p[fidx(M, i, j, k, 0)] = f;
    }
}

__global__ void __launch_bounds__(256) k_reflux(DFab U, DFab R, Box3 b, int dir, int side, int ncomp, double vol)
{
    int c[3];
    if (!box_thread3(b.lo, b.n, c[0], c[1], c[2])) return;
    int z[3] = { c[0], c[1], c[2] };
    if (side == 0) z[dir] -= 1;
    const double mult = side == 0 ? -1.0 : 1.0;
    for (int n = 0; n < ncomp; ++n)
        U.p[fidx(U, z[0], z[1], z[2], n)] += mult * R.p[fidx(R, c[0], c[1], c[2], n)] / vol;
}

__global__ void __launch_bounds__(256) k_lincomb(DFab D, DFab X, DFab Y, Box3 b, double a, double bb, int ncomp)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    for (int n = 0; n < ncomp; ++n)
        D.p[fidx(D, i, j, k, n)] = a * X.p[fidx(X, i, j, k, n)] + bb * Y.p[fidx(Y, i, j, k, n)];
}

// up to FABOPS_MAX independent region operations in one launch (castro_amd_fab_ops); op r owns threads [start[r], start[r+1])
#define FABOPS_MAX 16
struct FabOp { DFab D, X, Y; int lo[3], n[3]; int kind, dir, ncomp, side; double a, b;
               int flo[3], fhi[3]; };   // INTERP_CLEAN: lo / n enumerate the COARSE zones under the fine region [flo, fhi]
struct FabOps { int n; long start[FABOPS_MAX + 1]; FabOp op[FABOPS_MAX]; };
static_assert(sizeof(FabOps) + sizeof(DevParams) <= 4096, "k_fab_ops: the by-value table must fit the 4 KB of kernel arguments");

__device__ __forceinline__ void fab_op_thread(const FabOp& o, long t, const DevParams& P);

__global__ void __launch_bounds__(256) k_fab_ops(FabOps T, DevParams P)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= T.start[T.n]) return;
    int r = 0;
    while (tid >= T.start[r + 1]) ++r;
    fab_op_thread(T.op[r], tid - T.start[r], P);
}

// the same with the table in device memory (any number of operations): binary search of the thread's operation
__global__ void __launch_bounds__(256) k_fab_ops_mem(const FabOp* __restrict__ ops, const long* __restrict__ start, int n, DevParams P)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= start[n]) return;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= tid) lo = mid; else hi = mid - 1;
    }
    const FabOp o = ops[lo];
    fab_op_thread(o, tid - start[lo], P);
}

__device__ __forceinline__ void fab_op_thread(const FabOp& o, long t, const DevParams& P)
{
    int c[3];
    c[0] = o.lo[0] + (int)(t % o.n[0]);
    const long q = t / o.n[0];
    c[1] = o.lo[1] + (int)(q % o.n[1]);
    c[2] = o.lo[2] + (int)(q / o.n[1]);
    if (o.kind == CASTRO_AMD_OP_INTERP_CLEAN || o.kind == CASTRO_AMD_OP_INTERP) {
        // OP_INTERP: the interpolation alone, on the first o.ncomp (<= 8) components (Source_Type data: 7)
        const int nc = (o.kind == CASTRO_AMD_OP_INTERP) ? o.ncomp : NUM_STATE;
        // One thread per COARSE zone: the 27-point stencil, the three limited slopes and alpha of cc_interp_value are those of
        // all eight fine zones under it, so they are formed once (a thread per fine zone fetched 264 values for 8 results) and
        // evaluated at the children that lie inside the region -- the same expressions, the same bits.
        const DFab& C = o.X;
        double u[8][NUM_STATE];
#pragma unroll
        for (int n = 0; n < NUM_STATE; ++n) {
            if (n >= nc) continue;
#define CC(ii, jj, kk) C.p[fidx(C, c[0] + (ii), c[1] + (jj), c[2] + (kk), n)]
            const double u0 = CC(0, 0, 0);
            const double sx = mc_slope(CC(-1, 0, 0), u0, CC(1, 0, 0));
            const double sy = mc_slope(CC(0, -1, 0), u0, CC(0, 1, 0));
            const double sz = mc_slope(CC(0, 0, -1), u0, CC(0, 0, 1));
            double umax = u0, umin = u0;
            for (int kk = -1; kk <= 1; ++kk)
            for (int jj = -1; jj <= 1; ++jj)
            for (int ii = -1; ii <= 1; ++ii) {
                const double v = CC(ii, jj, kk);
                umax = amax(umax, v);
                umin = amin(umin, v);
            }
#undef CC
            const double dmax = 0.25 * (fabs(sx) + fabs(sy) + fabs(sz));
            double alpha = 1.0;
            if (dmax > umax - u0) alpha = amin(alpha, (umax - u0) / dmax);
            if (dmax > u0 - umin) alpha = amin(alpha, (u0 - umin) / dmax);
#pragma unroll
            for (int ch = 0; ch < 8; ++ch) {
                const double ox = (ch & 1) ? 0.25 : -0.25, oy = (ch & 2) ? 0.25 : -0.25, oz = (ch & 4) ? 0.25 : -0.25;
                u[ch][n] = u0 + alpha * (sx * ox + sy * oy + sz * oz);
            }
        }
        const int ntimes = (o.kind == CASTRO_AMD_OP_INTERP) ? 0 : (int)o.a;
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) {
            const int fi = 2 * c[0] + (ch & 1), fj = 2 * c[1] + ((ch >> 1) & 1), fk = 2 * c[2] + ((ch >> 2) & 1);
            if (fi < o.flo[0] || fi > o.fhi[0] || fj < o.flo[1] || fj > o.fhi[1] || fk < o.flo[2] || fk > o.fhi[2]) continue;
            if (ntimes > 0) clean_zone(P, ntimes, u[ch][URHO], u[ch][UMX], u[ch][UMY], u[ch][UMZ], u[ch][UEDEN], u[ch][UEINT], u[ch][UTEMP], u[ch][UFS]);
#pragma unroll
            for (int n = 0; n < NUM_STATE; ++n) if (n < nc) o.D.p[fidx(o.D, fi, fj, fk, n)] = u[ch][n];
        }
        return;
    }
    // CASTRO_AMD_OP_CLEAN never gets here: launch_fab_ops hands it to k_clean_state (launch_clean_state_boxes)
    if (o.kind == CASTRO_AMD_OP_AVGDOWN) {             // k_avgdown's arithmetic
        for (int n = 0; n < o.ncomp; ++n) {
            double s = 0.0;
            for (int kk = 0; kk < 2; ++kk)
            for (int jj = 0; jj < 2; ++jj)
            for (int ii = 0; ii < 2; ++ii) s += o.X.p[fidx(o.X, 2 * c[0] + ii, 2 * c[1] + jj, 2 * c[2] + kk, n)];
            o.D.p[fidx(o.D, c[0], c[1], c[2], n)] = 0.125 * s;
        }
        return;
    }
    if (o.kind == CASTRO_AMD_OP_REFLUX) {
        int z[3] = { c[0], c[1], c[2] };
        if (o.side == 0) z[o.dir] -= 1;
        const double mult = o.side == 0 ? -1.0 : 1.0;
        for (int n = 0; n < o.ncomp; ++n)
            o.D.p[fidx(o.D, z[0], z[1], z[2], n)] += mult * o.X.p[fidx(o.X, c[0], c[1], c[2], n)] / o.a;
        return;
    }
    if (o.kind == CASTRO_AMD_OP_FLUXREG_TO_FLUX) {      // k_fluxreg_to_flux's arithmetic; Y: the mass-flux FAB or none
        for (int n = 0; n < o.ncomp; ++n) {
            const long cf = fidx(o.D, c[0], c[1], c[2], n);
            const double f = o.D.p[cf] + o.X.p[fidx(o.X, c[0], c[1], c[2], n)];
            o.D.p[cf] = f;
            if (n == URHO && o.Y.p) o.Y.p[fidx(o.Y, c[0], c[1], c[2], 0)] = f;
        }
        return;
    }
    for (int n = 0; n < o.ncomp; ++n) {
        const long cd = fidx(o.D, c[0], c[1], c[2], n);
        if (o.kind == CASTRO_AMD_OP_COPY) {
            o.D.p[cd] = o.X.p[fidx(o.X, c[0], c[1], c[2], n)];
        } else if (o.kind == CASTRO_AMD_OP_LINCOMB) {
            o.D.p[cd] = o.a * o.X.p[fidx(o.X, c[0], c[1], c[2], n)] + o.b * o.Y.p[fidx(o.Y, c[0], c[1], c[2], n)];
        } else if (o.kind == CASTRO_AMD_OP_FLUXREG_CRSE_INIT) {
            o.D.p[cd] = o.a * o.X.p[fidx(o.X, c[0], c[1], c[2], n)];
        } else {
            const int dir = o.dir, t1 = (dir + 1) % 3, t2 = (dir + 2) % 3;
            int f[3];
            double s = 0.0;
            for (int bb = 0; bb < 2; ++bb)
            for (int aa = 0; aa < 2; ++aa) {
                f[dir] = 2 * c[dir];
                f[t1] = 2 * c[t1] + aa;
                f[t2] = 2 * c[t2] + bb;
                s += o.X.p[fidx(o.X, f[0], f[1], f[2], n)];
            }
            o.D.p[cd] += o.a * s;
        }
    }
}

int launch_fab_ops(int nops, const DFab* D, const DFab* X, const DFab* Y, const int* lo, const int* hi, const int* kind,
                   const int* dir, const int* side, const int* ncomp, const double* a, const double* b, hipStream_t stream, Profiler* prof,
                   const DevParams* Pp, StagedTable* arena)
{
    DevParams P;
    if (Pp) P = *Pp; else std::memset(&P, 0, sizeof(P));
    // CASTRO_AMD_OP_CLEAN operations go to k_clean_state, the one compiled copy of the plain clean sweep (see there), as tables
    // of their own, issued in front of the launches of the other kinds (the operations of a call are independent)
    {
        std::vector<DFab> cu;
        std::vector<int> clo, chi, cn;
        for (int r = 0; r < nops; ++r) {
            if (kind[r] != CASTRO_AMD_OP_CLEAN) continue;
            cu.push_back(D[r]);
            clo.insert(clo.end(), lo + 3 * r, lo + 3 * r + 3);
            chi.insert(chi.end(), hi + 3 * r, hi + 3 * r + 3);
            cn.push_back((int)a[r]);
        }
        if (!cu.empty()) {
            const int rc = launch_clean_state_boxes((int)cu.size(), cu.data(), clo.data(), chi.data(), cn.data(), P, stream, prof);
            if (rc != 0) return rc;
        }
    }
    auto fill = [&](FabOp& o, int r, long& n) {
        n = 1;
        if (kind[r] == CASTRO_AMD_OP_CLEAN) return false;
        int nn[3];
        for (int d = 0; d < 3; ++d) { nn[d] = hi[3 * r + d] - lo[3 * r + d] + 1; n *= nn[d] > 0 ? nn[d] : 0; }
        if (n <= 0) return false;
        o.D = D[r]; o.X = X[r]; o.Y = Y[r];
        for (int d = 0; d < 3; ++d) { o.lo[d] = lo[3 * r + d]; o.n[d] = nn[d]; o.flo[d] = lo[3 * r + d]; o.fhi[d] = hi[3 * r + d]; }
        if (kind[r] == CASTRO_AMD_OP_INTERP_CLEAN || kind[r] == CASTRO_AMD_OP_INTERP) {         // threads enumerate the coarse zones under the region
            n = 1;
            for (int d = 0; d < 3; ++d) {
                const int a_ = lo[3 * r + d], b_ = hi[3 * r + d];
                const int cl = a_ >= 0 ? a_ / 2 : -((-a_ + 1) / 2), ch = b_ >= 0 ? b_ / 2 : -((-b_ + 1) / 2);
                o.lo[d] = cl; o.n[d] = ch - cl + 1; n *= o.n[d];
            }
        }
        o.kind = kind[r]; o.dir = dir[r]; o.side = side[r]; o.ncomp = ncomp[r]; o.a = a[r]; o.b = b[r];
        return true;
    };
    if (arena && nops > FABOPS_MAX) {
        // one launch for the whole table: operations and their thread offsets go through a device buffer of the context
        // (pageable source: the runtime stages the bytes before hipMemcpyAsync returns; the copy is ordered on `stream`
        // behind the kernel that read the previous table)
        std::vector<FabOp> ops;
        std::vector<long> start(1, 0);
        ops.reserve(nops);
        for (int r = 0; r < nops; ++r) {
            FabOp o;
            long n;
            if (!fill(o, r, n)) continue;
            ops.push_back(o);
            start.push_back(start.back() + n);
        }
        if (ops.empty()) return 0;
        const FabOp* dops;
        const long* dstart;
        const int rt = arena->stage(ops.data(), ops.size(), start.data(), start.size(), stream, dops, dstart);
        if (rt != 0) return rt;
        static const char* const kind_name[10] = { "k_fab_ops_copy", "k_fab_ops_lincomb", "k_fab_ops_crse_init", "k_fab_ops_fine_add",
                                                   "k_fab_ops_reflux", "k_fab_ops_clean", "k_fab_ops_interp_clean", "k_fab_ops_avgdown",
                                                   "k_fab_ops_interp", "k_fab_ops_reg_to_flux" };
        prof_begin(prof, kind_name[ops[0].kind >= 0 && ops[0].kind < 10 ? ops[0].kind : 0], stream);     // tables are built per purpose: one kind each
        hipLaunchKernelGGL(k_fab_ops_mem, dim3((unsigned)((start.back() + 255) / 256)), dim3(256), 0, stream,
                           dops, dstart, (int)ops.size(), P);
        prof_end(prof, stream);
        return launch_status();
    }
    int done = 0;
    while (done < nops) {
        FabOps T;
        T.n = 0;
        T.start[0] = 0;
        for (; done < nops && T.n < FABOPS_MAX; ++done) {
            long n;
            if (!fill(T.op[T.n], done, n)) continue;
            T.start[T.n + 1] = T.start[T.n] + n;
            ++T.n;
        }
        if (T.n == 0) continue;
        prof_begin(prof, "k_fab_ops", stream);
        hipLaunchKernelGGL(k_fab_ops, dim3((unsigned)((T.start[T.n] + 255) / 256)), dim3(256), 0, stream, T, P);
        prof_end(prof, stream);
    }
    return launch_status();
}

__global__ void __launch_bounds__(256) k_error_tag(DFab Q, int comp, DFab T, Box3 b, int kind, double value)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
#define QQ(ii, jj, kk) Q.p[fidx(Q, ii, jj, kk, comp)]
    const double u = QQ(i, j, k);
    bool tag;
    if (kind == 0) tag = u >= value;
    else if (kind == 1) tag = u <= value;
    else {
        double ax = fabs(QQ(i + 1, j, k) - u); ax = amax(ax, fabs(u - QQ(i - 1, j, k)));
        double ay = fabs(QQ(i, j + 1, k) - u); ay = amax(ay, fabs(u - QQ(i, j - 1, k)));
        double az = fabs(QQ(i, j, k + 1) - u); az = amax(az, fabs(u - QQ(i, j, k - 1)));
        double g = amax(amax(ax, ay), az);
        tag = (kind == 2) ? (g >= value) : (g >= value * fabs(u));
    }
#undef QQ
    if (tag) T.p[fidx(T, i, j, k, 0)] = 1.0;
}

#define AMR_LAUNCH(name, kern, ...)                                                                     \
    long n; Box3 b = make_box3(lo, hi, n);                                                               \
    if (n <= 0) return 0;                                                                                \
    prof_begin(prof, name, stream);                                                                      \
    hipLaunchKernelGGL(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, __VA_ARGS__);      \
    prof_end(prof, stream);                                                                              \
    return launch_status()

int launch_cc_interp(const DFab& C, const DFab& F, const int lo[3], const int hi[3], int ncomp, hipStream_t stream, Profiler* prof)
{ AMR_LAUNCH("k_cc_interp", k_cc_interp, C, F, b, ncomp); }
int launch_avgdown(const DFab& F, const DFab& C, const int lo[3], const int hi[3], int ncomp, hipStream_t stream, Profiler* prof)
{ AMR_LAUNCH("k_avgdown", k_avgdown, F, C, b, ncomp); }
int launch_fluxreg(const DFab& R, const DFab& X, const int lo[3], const int hi[3], int dir, int ncomp, double mult, int mode,
                   hipStream_t stream, Profiler* prof)
{ AMR_LAUNCH("k_fluxreg", k_fluxreg, R, X, b, dir, ncomp, mult, mode); }
int launch_fluxreg_to_flux(const DFab& F, const DFab& R, const DFab& M, const int lo[3], const int hi[3], int ncomp,
                           hipStream_t stream, Profiler* prof)
{ AMR_LAUNCH("k_fluxreg_to_flux", k_fluxreg_to_flux, F, R, M, b, ncomp); }
int launch_reflux(const DFab& U, const DFab& R, const int lo[3], const int hi[3], int dir, int side, int ncomp, double vol,
                  hipStream_t stream, Profiler* prof)
{ AMR_LAUNCH("k_reflux", k_reflux, U, R, b, dir, side, ncomp, vol); }
int launch_error_tag(const DFab& Q, int comp, const DFab& T, const int lo[3], const int hi[3], int kind, double value,
                     hipStream_t stream, Profiler* prof)
{ AMR_LAUNCH("k_error_tag", k_error_tag, Q, comp, T, b, kind, value); }
int launch_lincomb(const DFab& D, const DFab& X, const DFab& Y, const int lo[3], const int hi[3], double a, double bb, int ncomp,
                   hipStream_t stream, Profiler* prof)
{ AMR_LAUNCH("k_lincomb", k_lincomb, D, X, Y, b, a, bb, ncomp); }

// ---------------------------------------------------------------------------------------
// derived plotfile fields (Source/driver/Derive.cpp); ids = CASTRO_AMD_DER_*
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_derive(DFab U, DFab D, int dcomp, Box3 b, int which, DevParams P,
                                                double dx0, double dx1, double dx2,
                                                double plo0, double plo1, double plo2, double c0, double c1, double c2)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
#define UU(ii, jj, kk, n) U.p[fidx(U, ii, jj, kk, n)]
    const double rho = UU(i, j, k, URHO);
    // the eos_input_re call of the EOS-based derives (Derive.cpp:37-50)
    const double rhoInv = 1.0 / rho;
    const double e = UU(i, j, k, UEINT) * rhoInv;
    const double p = (P.gamma - 1.0) * rho * e;
    const double cs = sqrt(P.gamma * p / rho);
    const double mx = UU(i, j, k, UMX), my = UU(i, j, k, UMY), mz = UU(i, j, k, UMZ);
    double v = 0.0;
    switch (which) {
    case 0: v = p; break;
    case 1: v = 0.5 / rho * (mx * mx + my * my + mz * mz); break;
    case 2: v = cs; break;
    case 3: v = P.gamma; break;
    case 4: v = sqrt(mx * mx + my * my + mz * mz) / rho / cs; break;
    case 5: {
        double vx = 0.5 * (UU(i + 1, j, k, UMY) / UU(i + 1, j, k, URHO) - UU(i - 1, j, k, UMY) / UU(i - 1, j, k, URHO)) / dx0;
        double wx = 0.5 * (UU(i + 1, j, k, UMZ) / UU(i + 1, j, k, URHO) - UU(i - 1, j, k, UMZ) / UU(i - 1, j, k, URHO)) / dx0;
        double uy = 0.5 * (UU(i, j + 1, k, UMX) / UU(i, j + 1, k, URHO) - UU(i, j - 1, k, UMX) / UU(i, j - 1, k, URHO)) / dx1;
        double wy = 0.5 * (UU(i, j + 1, k, UMZ) / UU(i, j + 1, k, URHO) - UU(i, j - 1, k, UMZ) / UU(i, j - 1, k, URHO)) / dx1;
        double uz = 0.5 * (UU(i, j, k + 1, UMX) / UU(i, j, k + 1, URHO) - UU(i, j, k - 1, UMX) / UU(i, j, k - 1, URHO)) / dx2;
        double vz = 0.5 * (UU(i, j, k + 1, UMY) / UU(i, j, k + 1, URHO) - UU(i, j, k - 1, UMY) / UU(i, j, k - 1, URHO)) / dx2;
        double v1 = wy - vz, v2 = uz - wx, v3 = vx - uy;
        v = sqrt(v1 * v1 + v2 * v2 + v3 * v3);
        break; }
    case 6: {
        double uhi = UU(i + 1, j, k, UMX) / UU(i + 1, j, k, URHO);
        double ulo = UU(i - 1, j, k, UMX) / UU(i - 1, j, k, URHO);
        double vhi = UU(i, j + 1, k, UMY) / UU(i, j + 1, k, URHO);
        double vlo = UU(i, j - 1, k, UMY) / UU(i, j - 1, k, URHO);
        double whi = UU(i, j, k + 1, UMZ) / UU(i, j, k + 1, URHO);
        double wlo = UU(i, j, k - 1, UMZ) / UU(i, j, k - 1, URHO);
        v = 0.5 * (uhi - ulo) / dx0;
        v += 0.5 * (vhi - vlo) / dx1;
        v += 0.5 * (whi - wlo) / dx2;
        break; }
    case 7: {
        double ux = mx * rhoInv, uy = my * rhoInv, uz = mz * rhoInv;
        v = UU(i, j, k, UEDEN) * rhoInv - 0.5 * (ux * ux + uy * uy + uz * uz);
        break; }
    case 8: v = UU(i, j, k, UEINT) / rho; break;
    case 9: v = log10(rho); break;
    case 10: v = UU(i, j, k, UFS) / rho; break;
    case 11: {
        double sum = 0.0;
        double xn = UU(i, j, k, UFS) / rho;
        sum += xn / P.abar;
        v = 1.0 / sum;
        break; }
    case 12: v = mx / rho; break;
    case 13: v = my / rho; break;
    case 14: v = mz / rho; break;
    case 15: v = sqrt((mx * mx + my * my + mz * mz)) * rhoInv; break;
    case 16: {
        double x = plo0 + ((double)i + 0.5) * dx0 - c0;
        double y = plo1 + ((double)j + 0.5) * dx1 - c1;
        double z = plo2 + ((double)k + 0.5) * dx2 - c2;
        double r = sqrt(x * x + y * y + z * z);
        v = (mx * x + my * y + mz * z) / (rho * r);
        break; }
    case 17: v = sqrt(mx * mx + my * my + mz * mz); break;
    case 18: v = rho; break;
    case 19: v = UU(i, j, k, UTEMP); break;
    case 20: v = UU(i, j, k, UFS) / rho; break;
    case 21: {
        double x = plo0 + ((double)i + 0.5) * dx0 - c0;
        double y = plo1 + ((double)j + 0.5) * dx1 - c1;
        double z = plo2 + ((double)k + 0.5) * dx2 - c2;
        double r = sqrt(x * x + y * y + z * z);
        double vtot2 = (mx * mx + my * my + mz * mz) / (rho * rho);
        double vr = (mx * x + my * y + mz * z) / (rho * r);
        v = sqrt(amax(vtot2 - vr * vr, 0.0));
        break; }
    case 22: case 23: case 24: {
        double loc0 = plo0 + (0.5 + (double)i) * dx0;
        double loc1 = plo1 + (0.5 + (double)j) * dx1;
        double loc2 = plo2 + (0.5 + (double)k) * dx2;
        loc0 -= c0; loc1 -= c1; loc2 -= c2;
        if (which == 22) v = loc1 * mz - loc2 * my;
        else if (which == 23) v = loc2 * mx - loc0 * mz;
        else v = loc0 * my - loc1 * mx;
        break; }
    }
#undef UU
    D.p[fidx(D, i, j, k, dcomp)] = v;
}

int launch_derive(int which, const DFab& U, const DFab& D, int dcomp, const int lo[3], const int hi[3],
                  const double dx[3], const double problo[3], const DevParams& P, const double center[3],
                  hipStream_t stream, Profiler* prof)
{
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    prof_begin(prof, "k_derive", stream);
    hipLaunchKernelGGL(k_derive, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, U, D, dcomp, b, which, P,
                       dx[0], dx[1], dx[2], problo[0], problo[1], problo[2], center[0], center[1], center[2]);
    prof_end(prof, stream);
    return launch_status();
}

// ---------------------------------------------------------------------------------------
// physical-boundary ghost fill (AMReX GpuBndryFuncFab semantics [3P], SURVEY.md D.2;
// Castro BC tables Source/driver/Castro_setup.cpp:40-53; EXT_DIR -> FOEXTRAP per
// Source/problems/Castro_bc_fill_nd.cpp:26-39).  One launch per (direction, side).
// kind: 0 first-order extrapolation, +1 reflect even, -1 reflect odd (normal momentum).
// ---------------------------------------------------------------------------------------
// One launch for all faces, edges and corners: the x, y, z sweeps of the reference (each over the full extent
// already filled, so edges and corners inherit from filled neighbours) compose to an independent index map per
// direction -- clamp to the nearest interior zone (FOEXTRAP) or mirror about the boundary (walls), with the normal
// momentum of every mirrored direction negated -- applied to the zones outside the domain in a non-periodic direction.
struct BcMap { int lo[3], hi[3]; int kind_lo[3], kind_hi[3]; };   // domain extent; kind 0 leave (interior), 1 extrapolate, 2 wall

__global__ void __launch_bounds__(256) k_bc_fill(DFab U, Slabs S, int ncomp, BcMap M)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= S.start[6]) return;
    int r = 0;
    while (tid >= S.start[r + 1]) ++r;
    const long t = tid - S.start[r];
    const int n0 = S.nn[r][0], n1 = S.nn[r][1];
    int ijk[3];
    ijk[0] = S.lo[r][0] + (int)(t % n0);
    const long q = t / n0;
    ijk[1] = S.lo[r][1] + (int)(q % n1);
    ijk[2] = S.lo[r][2] + (int)(q / n1);
    int s[3];
    bool flip[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        s[d] = ijk[d];
        flip[d] = false;
        if (ijk[d] < M.lo[d] && M.kind_lo[d] != 0) {
            if (M.kind_lo[d] == 1) s[d] = M.lo[d];
            else { s[d] = 2 * M.lo[d] - ijk[d] - 1; flip[d] = true; }
        } else if (ijk[d] > M.hi[d] && M.kind_hi[d] != 0) {
            if (M.kind_hi[d] == 1) s[d] = M.hi[d];
            else { s[d] = 2 * M.hi[d] - ijk[d] + 1; flip[d] = true; }
        }
    }
    const long cd = fidx(U, ijk[0], ijk[1], ijk[2], 0);
    const long cs = fidx(U, s[0], s[1], s[2], 0);
    for (int n = 0; n < ncomp; ++n) {
        double v = U.p[cs + U.sn * n];
        if (n >= UMX && n <= UMZ && flip[n - UMX]) v = -v;      // norm_vel_bc: REFLECT_ODD
        U.p[cd + U.sn * n] = v;
    }
}

static int launch_bc_fill_map(const DFab& U, const int flo[3], const int fhi[3], int ncomp, const BcMap& M,
                              hipStream_t stream, Profiler* prof);

int launch_bc_fill(const DFab& U, const int flo[3], const int fhi[3], int ncomp, const DevGeom& g,
                   const int lo_bc[3], const int hi_bc[3], hipStream_t stream, Profiler* prof)
{
    BcMap M;
    bool degenerate = false;       // a mirrored ghost layer reaches past the other side of the domain
    for (int d = 0; d < 3; ++d) {
        M.lo[d] = g.domlo[d]; M.hi[d] = g.domhi[d];
        M.kind_lo[d] = lo_bc[d] == 0 ? 0 : (lo_bc[d] >= 3 ? 2 : 1);      // Symmetry, SlipWall, NoSlipWall mirror
        M.kind_hi[d] = hi_bc[d] == 0 ? 0 : (hi_bc[d] >= 3 ? 2 : 1);
        const int ndom = g.domhi[d] - g.domlo[d] + 1;
        if (M.kind_lo[d] == 2 && g.domlo[d] - flo[d] > ndom) degenerate = true;
        if (M.kind_hi[d] == 2 && fhi[d] - g.domhi[d] > ndom) degenerate = true;
    }
    if (!degenerate) return launch_bc_fill_map(U, flo, fhi, ncomp, M, stream, prof);
    // a domain narrower than the ghost depth in a mirrored direction: the sweeps read zones that other sweeps
    // write, so they are issued one (direction, side) at a time in the reference's order
    for (int d = 0; d < 3; ++d)
        for (int side = 0; side < 2; ++side) {
            BcMap one = M;
            for (int e = 0; e < 3; ++e) { one.kind_lo[e] = 0; one.kind_hi[e] = 0; }
            if (side == 0) one.kind_lo[d] = M.kind_lo[d]; else one.kind_hi[d] = M.kind_hi[d];
            int rc = launch_bc_fill_map(U, flo, fhi, ncomp, one, stream, prof);
            if (rc != 0) return rc;
        }
    return 0;
}

static int launch_bc_fill_map(const DFab& U, const int flo[3], const int fhi[3], int ncomp, const BcMap& M,
                              hipStream_t stream, Profiler* prof)
{
    int blo[3], bhi[3];        // the part of the FAB that needs no physical-boundary fill
    for (int d = 0; d < 3; ++d) {
        blo[d] = (M.kind_lo[d] != 0 && flo[d] < M.lo[d]) ? M.lo[d] : flo[d];
        bhi[d] = (M.kind_hi[d] != 0 && fhi[d] > M.hi[d]) ? M.hi[d] : fhi[d];
        if (blo[d] > bhi[d]) return 0;                                      // FAB entirely outside the domain: nothing to copy from
    }
    const Slabs S = shell_slabs(flo, fhi, blo, bhi);      // the FAB box minus [blo, bhi]
    if (S.start[6] <= 0) return 0;
    prof_begin(prof, "k_bc_fill", stream);
    hipLaunchKernelGGL(k_bc_fill, dim3((unsigned)((S.start[6] + 255) / 256)), dim3(256), 0, stream, U, S, ncomp, M);
    prof_end(prof, stream);
    return launch_status();
}

// ---------------------------------------------------------------------------------------
// FAB region copy and halo pack/unpack
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_copy(DFab dst, DFab src, Box3 b, int ncomp)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    const long cd = fidx(dst, i, j, k, 0), cs = fidx(src, i, j, k, 0);
    for (int n = 0; n < ncomp; ++n) dst.p[cd + dst.sn * n] = src.p[cs + src.sn * n];
}

int launch_copy(const DFab& dst, const DFab& src, const int lo[3], const int hi[3], int ncomp,
                hipStream_t stream, Profiler* prof)
{
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    prof_begin(prof, "k_copy", stream);
    hipLaunchKernelGGL(k_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dst, src, b, ncomp);
    prof_end(prof, stream);
    return launch_status();
}

__global__ void __launch_bounds__(256) k_pack(DFab f, Box3 b, int ncomp, double* buf, int unpack)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;
    const long cf = fidx(f, i, j, k, 0);
    const long nb = (long)b.n[0] * b.n[1] * b.n[2];
    const long cb = (long)(i - b.lo[0]) + (long)b.n[0] * ((long)(j - b.lo[1]) + (long)b.n[1] * (long)(k - b.lo[2]));
    if (unpack) {
        for (int n = 0; n < ncomp; ++n) f.p[cf + f.sn * n] = buf[cb + nb * n];
    } else {
        for (int n = 0; n < ncomp; ++n) buf[cb + nb * n] = f.p[cf + f.sn * n];
    }
}

int launch_pack(const DFab& f, const int lo[3], const int hi[3], int ncomp, double* buf, int unpack,
                hipStream_t stream, Profiler* prof)
{
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    prof_begin(prof, unpack ? "k_unpack" : "k_pack", stream);
    hipLaunchKernelGGL(k_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, f, b, ncomp, buf, unpack);
    prof_end(prof, stream);
    return launch_status();
}

// All halo regions of one FillBoundary in one launch: region r owns threads [start[r], start[r+1]) and the
// doubles buf[off[r] ...] (same ordering as k_pack, restricted to the region).
struct PackRegions {
    int n;
    int lo[CASTRO_AMD_MAX_REGIONS][3], nn[CASTRO_AMD_MAX_REGIONS][3];
    long off[CASTRO_AMD_MAX_REGIONS];
    long start[CASTRO_AMD_MAX_REGIONS + 1];
};

__global__ void __launch_bounds__(256) k_pack_regions(DFab f, PackRegions R, int ncomp, double* buf, int unpack)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= R.start[R.n]) return;
    int r = 0;
    while (tid >= R.start[r + 1]) ++r;
    const long t = tid - R.start[r];
    const int n0 = R.nn[r][0], n1 = R.nn[r][1];
    const int ii = (int)(t % n0);
    const long q = t / n0;
    const int jj = (int)(q % n1), kk = (int)(q / n1);
    const long cf = fidx(f, R.lo[r][0] + ii, R.lo[r][1] + jj, R.lo[r][2] + kk, 0);
    const long nb = (long)n0 * n1 * R.nn[r][2];
    double* b = buf + R.off[r] + t;
    if (unpack) {
        for (int n = 0; n < ncomp; ++n) f.p[cf + f.sn * n] = b[nb * n];
    } else {
        for (int n = 0; n < ncomp; ++n) b[nb * n] = f.p[cf + f.sn * n];
    }
}

int launch_pack_regions(const DFab& f, int nreg, const int* lo, const int* hi, const long long* off, int ncomp, double* buf,
                        int unpack, hipStream_t stream, Profiler* prof)
{
    PackRegions R;
    R.n = 0;
    R.start[0] = 0;
    for (int r = 0; r < nreg; ++r) {
        long n = 1;
        int nn[3];
        for (int d = 0; d < 3; ++d) { nn[d] = hi[3 * r + d] - lo[3 * r + d] + 1; n *= nn[d] > 0 ? nn[d] : 0; }
        if (n <= 0) continue;
        const int m = R.n++;
        for (int d = 0; d < 3; ++d) { R.lo[m][d] = lo[3 * r + d]; R.nn[m][d] = nn[d]; }
        R.off[m] = (long)off[r];
        R.start[m + 1] = R.start[m] + n;
    }
    if (R.n == 0) return 0;
    prof_begin(prof, unpack ? "k_unpack" : "k_pack", stream);
    hipLaunchKernelGGL(k_pack_regions, dim3((unsigned)((R.start[R.n] + 255) / 256)), dim3(256), 0, stream, f, R, ncomp, buf, unpack);
    prof_end(prof, stream);
    return launch_status();
}

// ---------------------------------------------------------------------------------------
// Sedov initial data (Exec/hydro_tests/Sedov/problem_initialize_state_data.H:8-148, Cartesian)
// ---------------------------------------------------------------------------------------
struct V3 { double v[3]; };

__global__ void __launch_bounds__(256) k_sedov_init(DFab U, Box3 b, V3 dx, V3 problo, V3 center,
                                                    double r_init, double e_exp, double e_ambient,
                                                    double temp_ambient, double dens_ambient, int nsub)
{
    int i, j, k;
    if (!box_thread3(b.lo, b.n, i, j, k)) return;

    const double ds0 = dx.v[0] / nsub, ds1 = dx.v[1] / nsub, ds2 = dx.v[2] / nsub;
    const double xmin = problo.v[0] + dx.v[0] * (double)i;
    const double ymin = problo.v[1] + dx.v[1] * (double)j;
    const double zmin = problo.v[2] + dx.v[2] * (double)k;

    double vol_pert = 0.0, vol_ambient = 0.0;

    for (int kk = 0; kk <= nsub - 1; ++kk) {
        double zz = zmin + ds2 * ((double)kk + 0.5);
        for (int jj = 0; jj <= nsub - 1; ++jj) {
            double yy = ymin + ds1 * ((double)jj + 0.5);
            for (int ii = 0; ii <= nsub - 1; ++ii) {
                double xx = xmin + ds0 * ((double)ii + 0.5);
                double dist = (center.v[0] - xx) * (center.v[0] - xx) +
                              (center.v[1] - yy) * (center.v[1] - yy) +
                              (center.v[2] - zz) * (center.v[2] - zz);
                if (dist <= r_init * r_init) vol_pert = vol_pert + 1.0;
                else vol_ambient = vol_ambient + 1.0;
            }
        }
    }

    double e_zone = (vol_pert * e_exp + vol_ambient * e_ambient) / (vol_pert + vol_ambient);
    double eint = dens_ambient * e_zone;

    const long c = fidx(U, i, j, k, 0);
    const double rho = dens_ambient, mx = 0.e0, my = 0.e0, mz = 0.e0;
    U.p[c + U.sn * URHO] = rho;
    U.p[c + U.sn * UMX] = mx;
    U.p[c + U.sn * UMY] = my;
    U.p[c + U.sn * UMZ] = mz;
    U.p[c + U.sn * UEDEN] = eint + 0.5e0 * (mx * mx / rho + my * my / rho + mz * mz / rho);
    U.p[c + U.sn * UEINT] = eint;
    U.p[c + U.sn * UTEMP] = temp_ambient;
    U.p[c + U.sn * UFS] = rho;
}

int launch_sedov_init(const DFab& U, const int lo[3], const int hi[3], const DevParams& P,
                      const double dx[3], const double problo[3], const double center[3],
                      double r_init, double e_exp, double e_ambient, double temp_ambient,
                      double dens_ambient, int nsub, hipStream_t stream, Profiler* prof)
{
    (void)P;
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    V3 vdx, vlo, vc;
    for (int d = 0; d < 3; ++d) { vdx.v[d] = dx[d]; vlo.v[d] = problo[d]; vc.v[d] = center[d]; }
    prof_begin(prof, "k_sedov_init", stream);
    hipLaunchKernelGGL(k_sedov_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, U, b, vdx, vlo, vc,
                       r_init, e_exp, e_ambient, temp_ambient, dens_ambient, nsub);
    prof_end(prof, stream);
    return launch_status();
}

// Sod initial data (Exec/hydro_tests/Sod/problem_initialize_state_data.H)
__global__ void __launch_bounds__(256) k_sod_init(DFab U, Box3 b, V3 dx, V3 problo, double split, int idir0,
                                                  double rho_l, double u_l, double rhoe_l, double T_l,
                                                  double rho_r, double u_r, double rhoe_r, double T_r)
{
    int ijk[3];
    if (!box_thread3(b.lo, b.n, ijk[0], ijk[1], ijk[2])) return;
    const double x = problo.v[idir0] + dx.v[idir0] * ((double)ijk[idir0] + 0.5);
    const bool left = x <= split;
    const double rho = left ? rho_l : rho_r;
    const double u = left ? u_l : u_r;
    const double rhoe = left ? rhoe_l : rhoe_r;
    const long c = fidx(U, ijk[0], ijk[1], ijk[2], 0);
    U.p[c + U.sn * URHO] = rho;
    U.p[c + U.sn * UMX] = 0.0;
    U.p[c + U.sn * UMY] = 0.0;
    U.p[c + U.sn * UMZ] = 0.0;
    U.p[c + U.sn * (UMX + idir0)] = rho * u;
    U.p[c + U.sn * UEDEN] = rhoe + 0.5 * rho * u * u;
    U.p[c + U.sn * UEINT] = rhoe;
    U.p[c + U.sn * UTEMP] = left ? T_l : T_r;
    U.p[c + U.sn * UFS] = rho;
}

int launch_sod_init(const DFab& U, const int lo[3], const int hi[3], const double dx[3],
                    const double problo[3], double split, int idir0,
                    double rho_l, double u_l, double rhoe_l, double T_l,
                    double rho_r, double u_r, double rhoe_r, double T_r,
                    hipStream_t stream, Profiler* prof)
{
    Box3 b;
    long n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    if (n <= 0) return 0;
    V3 vdx, vlo;
    for (int d = 0; d < 3; ++d) { vdx.v[d] = dx[d]; vlo.v[d] = problo[d]; }
    prof_begin(prof, "k_sod_init", stream);
    hipLaunchKernelGGL(k_sod_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, U, b, vdx, vlo, split,
                       idir0, rho_l, u_l, rhoe_l, T_l, rho_r, u_r, rhoe_r, T_r);
    prof_end(prof, stream);
    return launch_status();
}

} // namespace cad

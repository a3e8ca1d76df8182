// extbc_kernels.hip -- the second half of the physical-boundary fill of the state (ca_statefill,
// Source/problems/Castro_bc_fill_nd.cpp:41-105), 3-D Cartesian, gamma-law EOS:
//   k_ambient_fill   ambient_fill (Source/problems/ambient_fill.cpp:61-154): the zones beyond an Outflow face take
//                    ambient::ambient_state; with castro.ambient_outflow_vel the outgoing part of the normal momentum of the
//                    first zone inside the domain
//   k_hse_fill       hse_fill (Source/problems/hse_fill.cpp): every ghost column of an Inflow face of type HSE
//                    (Source/problems/ext_bc_types.H) is integrated outward in hydrostatic equilibrium under gravity.const_grav
// Both work in place on a FAB whose zones outside the domain hold the generic fill (k_bc_fill) already; the ambient launch
// comes first on the same stream, because an HSE column in a transverse ghost row starts from a zone it may have written.
//
// The order inside ambient_fill.  Without ambient_outflow_vel a zone reads nothing: one launch.  With it, a zone reads the
// normal momentum of the domain's edge zone of its line, and that zone can itself lie beyond another ambient face.  The
// reference's CPU loop (k outermost, i innermost, ascending) then gives
//   * on a LOW face the value from before the ambient fill: the edge zone has the larger index and is visited later;
//   * on a HIGH face the value from after it: 0, because the `else if` chain of an ambient zone with that index inside the
//     domain zeroes that momentum, whichever later branch it takes;
// (the reference's GPU build races there).  The kernels give the CPU's answer whatever the thread order: the high faces test
// whether the edge zone is an ambient zone instead of reading what another thread writes, and the low faces read before any
// writer runs -- the zones of the chain's x branch read only zones of its y and z branches or of the domain, those of the y
// branch only zones of the z branch or of the domain, so the branches go in three launches x, y, z.
//
// Numerics.  The fill uses + - * / min max abs only.  `exact` build (-ffp-contract=off, IEEE division): the expressions of the
// reference in its order -- the bits of the numpy restatement (tests/ext_bc_ref.py) and of the reference's own files run on the
// CPU (tools/stub_probe/probe_bc.cpp).  `contract` build: the same source under that build's flags.
// eos(eos_input_rt) is the gamma-law gas of hydro_device.h, and dpdr = p / rho: Microphysics' EOS/gamma_law [3P], not in the
// reference tree.
#include <hip/hip_runtime.h>
#include "../../include/castro_hydro_amd.h"
#include "hydro_device.h"
#include "ctu_kernels.h"

namespace cad {

namespace {

constexpr int HSE_MAX_ITER = 250;          // ext_bc_types.H: hse::MAX_ITER, hse::TOL
constexpr double HSE_TOL = 1.e-8;
constexpr int BC_INFLOW = 1, BC_OUTFLOW = 2;       // phys_bc: EXT_DIR, FOEXTRAP (Castro_setup.cpp:40-53)
constexpr int EXT_HSE = 1;

struct AmbDev {
    int domlo[3], domhi[3];
    int amb_lo[3], amb_hi[3];         // the face is an ambient face
    int outflow_vel;
    double state[NUM_STATE];
};

__device__ __forceinline__ bool beyond_ambient_face(const AmbDev& A, const int ijk[3])
{
    return (A.amb_lo[0] && ijk[0] < A.domlo[0]) || (A.amb_hi[0] && ijk[0] > A.domhi[0]) ||
           (A.amb_lo[1] && ijk[1] < A.domlo[1]) || (A.amb_hi[1] && ijk[1] > A.domhi[1]) ||
           (A.amb_lo[2] && ijk[2] < A.domlo[2]) || (A.amb_hi[2] && ijk[2] > A.domhi[2]);
}

// One thread per zone of the slabs (every one of them lies beyond an ambient face).  branch: -1 every zone (no zone reads
// another), else only the zones that take the x (0), y (1) or z (2) branch of the reference's `else if` chain
__global__ void __launch_bounds__(256) k_ambient_fill(DFab U, Slabs S, AmbDev A, int branch)
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

    double u[NUM_STATE];
#pragma unroll
    for (int n = 0; n < NUM_STATE; ++n) u[n] = A.state[n];

    if (A.outflow_vel == 1) {
        // the chain x low, x high, y low, y high, z low, z high: it asks where the zone is, not whether that face is ambient
        int d = 0;
        while (d < 3 && ijk[d] >= A.domlo[d] && ijk[d] <= A.domhi[d]) ++d;
        if (d != branch) return;
        const bool low = ijk[d] < A.domlo[d];
        int s[3] = { ijk[0], ijk[1], ijk[2] };
        s[d] = low ? A.domlo[d] : A.domhi[d];
        // extrapolate the normal velocity only if it is outgoing
        double mom;
        if (low) {
            mom = amin(0.0, U.p[(long)(s[0] - U.lo[0]) + U.sy * (long)(s[1] - U.lo[1]) + U.sz * (long)(s[2] - U.lo[2]) + U.sn * (UMX + d)]);
        } else {
            const double edge = beyond_ambient_face(A, s)
                ? 0.0 : U.p[(long)(s[0] - U.lo[0]) + U.sy * (long)(s[1] - U.lo[1]) + U.sz * (long)(s[2] - U.lo[2]) + U.sn * (UMX + d)];
            mom = amax(0.0, edge);
        }
        u[UMX] = 0.0; u[UMY] = 0.0; u[UMZ] = 0.0;
        u[UMX + d] = mom;
        // now make the energy consistent
        u[UEDEN] = u[UEINT] + 0.5 * (u[UMX] * u[UMX] + u[UMY] * u[UMY] + u[UMZ] * u[UMZ]) / u[URHO];
    }

    double* p = U.p + ((long)(ijk[0] - U.lo[0]) + U.sy * (long)(ijk[1] - U.lo[1]) + U.sz * (long)(ijk[2] - U.lo[2]));
#pragma unroll
    for (int n = 0; n < NUM_STATE; ++n) p[U.sn * n] = u[n];
}

// one active HSE face: direction, side (0 low, 1 high), and its ghost columns -- the FAB's whole extent in the two other
// directions t0 < t1, tn[0] x tn[1] columns from tlo, the threads [start, start + tn[0] * tn[1]) of the launch
struct HseFace { int dir, side; int tlo[2], tn[2]; long start; };
struct HseDev {
    HseFace f[6];
    int nface;
    long ntot;
    int zero_vels, interp_temp, reflect_vels;
    double const_grav;
    double dx[3];
    int domlo[3], domhi[3];
    int flo[3], fhi[3];
};

// the zone with index ii along D and (a, b) along the two other directions, component 0
template <int D> __device__ __forceinline__ long column_zone(const DFab& U, int ii, int a, int b)
{
    const int i = D == 0 ? ii : a, j = D == 1 ? ii : (D == 0 ? a : b), k = D == 2 ? ii : b;
    return (long)(i - U.lo[0]) + U.sy * (long)(j - U.lo[1]) + U.sz * (long)(k - U.lo[2]);
}

// The walk of one ghost column of the low (HI = false) or the high (HI = true) face of direction D.  The reference writes the
// six faces out one after the other; they are the same text with the indices exchanged, except for what the two sides of a
// direction differ in, and that is written out here as there: below the domain p_want = p_above - dx/2 (rho + rho_above) g and
// the Newton denominator is dpdr + dx/2 g, above it the two signs are exchanged; the mirror zone of the reflected normal
// momentum is domlo + off / domhi - off; the temperature is extrapolated from ii + 1, ii + 2 / ii - 1, ii - 2.  One face differs
// in more than that: z low stores the temperature in one zone only (below).
// Returns whether every zone of the column converged.
template <int D, bool HI>
__device__ bool hse_column(const DFab& U, const HseDev& T, const DevParams& P, int a, int b)
{
    const int dom = HI ? T.domhi[D] : T.domlo[D];
    const int end = HI ? T.fhi[D] : T.flo[D];
    const int step = HI ? 1 : -1;
    const long sn = U.sn;
    const double dx = T.dx[D], grav = T.const_grav;
    const long c0 = column_zone<D>(U, dom, a, b);

    double dens_prev = U.p[c0 + sn * URHO];                 // dens_above / dens_below
    const double temp_prev = U.p[c0 + sn * UTEMP];
    const double X_zone = U.p[c0 + sn * UFS] / dens_prev;
    const double dens_base = dens_prev;                     // the density at the base (top) of the domain
    const double mom_base[3] = { U.p[c0 + sn * UMX], U.p[c0 + sn * UMY], U.p[c0 + sn * UMZ] };
    // the pressure of the first zone inside the domain
    double pres_prev = (P.gamma - 1.0) * dens_prev * eos_e_of_T(P, temp_prev, X_zone);
    bool all_converged = true;

    for (int ii = dom + step; HI ? ii <= end : ii >= end; ii += step) {
        const long c = column_zone<D>(U, ii, a, b);
        double dens_zone = dens_prev;                        // initial guess
        // temperature and species held constant in BCs
        double temp_zone;
        if (T.interp_temp == 1) {
            temp_zone = 2 * U.p[column_zone<D>(U, ii - step, a, b) + sn * UTEMP] - U.p[column_zone<D>(U, ii - 2 * step, a, b) + sn * UTEMP];
        } else {
            temp_zone = temp_prev;
        }
        const double e_zone = eos_e_of_T(P, temp_zone, X_zone);       // eos_input_rt: e depends on T and X alone
        bool converged_hse = false;
        for (int iter = 0; iter < HSE_MAX_ITER; ++iter) {
            // pressure needed from HSE
            double p_want, denom_grav;
            if (HI) p_want = pres_prev + dx * 0.5 * (dens_zone + dens_prev) * grav;
            else    p_want = pres_prev - dx * 0.5 * (dens_zone + dens_prev) * grav;
            // pressure from EOS
            const double pres_zone = (P.gamma - 1.0) * dens_zone * e_zone;
            const double dpdr = pres_zone / dens_zone;
            // Newton-Raphson - we want to zero A = p_want - p(rho)
            const double A = p_want - pres_zone;
            if (HI) denom_grav = dpdr - 0.5 * dx * grav;
            else    denom_grav = dpdr + 0.5 * dx * grav;
            const double drho = A / denom_grav;
            dens_zone = amax(0.9 * dens_zone, amin(dens_zone + drho, 1.1 * dens_zone));
            if (fabs(drho) < HSE_TOL * dens_zone) { converged_hse = true; break; }
        }
        if (!converged_hse) all_converged = false;           // the zone takes the last iterate, as on the reference's GPU build

        double mom[3];
        if (T.zero_vels == 1) {
            mom[0] = 0.0; mom[1] = 0.0; mom[2] = 0.0;
        } else if (T.reflect_vels == 1) {
            // the normal momentum of the zone mirrored about the boundary, over that zone's own density; the transverse momenta
            // of the base zone with a minus sign too, as the reference has them
            const int off = HI ? ii - dom - 1 : dom - ii - 1;
            const long cm = column_zone<D>(U, HI ? dom - off : dom + off, a, b);
#pragma unroll
            for (int m = 0; m < 3; ++m)
                mom[m] = m == D ? -dens_zone * (U.p[cm + sn * (UMX + D)] / U.p[cm + sn * URHO]) : -dens_zone * (mom_base[m] / dens_base);
        } else {
            // zero gradient
#pragma unroll
            for (int m = 0; m < 3; ++m) mom[m] = dens_zone * (mom_base[m] / dens_base);
        }

        const double pres_zone = (P.gamma - 1.0) * dens_zone * e_zone;
        // store the final state
        U.p[c + sn * UMX] = mom[0];
        U.p[c + sn * UMY] = mom[1];
        U.p[c + sn * UMZ] = mom[2];
        U.p[c + sn * URHO] = dens_zone;
        U.p[c + sn * UEINT] = dens_zone * e_zone;
        U.p[c + sn * UEDEN] = dens_zone * e_zone + 0.5 * (mom[0] * mom[0] + mom[1] * mom[1] + mom[2] * mom[2]) / dens_zone;
        // the z-low face of the reference stores the temperature at the index of its ParallelFor -- the FIRST ghost zone --
        // for every zone of the walk (hse_fill.cpp:963: adv(i,j,k,UTEMP), not kk); the deeper zones keep what the generic fill
        // gave them, and the extrapolation of hse_interp_temp reads what this leaves.  The four other faces store it in the zone
        U.p[((D == 2 && !HI) ? column_zone<D>(U, dom - 1, a, b) : c) + sn * UTEMP] = temp_zone;
        U.p[c + sn * UFS] = dens_zone * X_zone;
        // for the next zone
        dens_prev = dens_zone;
        pres_prev = pres_zone;
    }
    return all_converged;
}

// One thread per ghost column of the faces of the table.  On a z face the lanes of a wave run along x (unit stride); on an x
// face they run along y and are a row apart.
__global__ void __launch_bounds__(256) k_hse_fill(DFab U, HseDev T, DevParams P, int* __restrict__ unconverged)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= T.ntot) return;
    int f = 0;
    while (f + 1 < T.nface && tid >= T.f[f + 1].start) ++f;
    const HseFace F = T.f[f];
    const long t = tid - F.start;
    const int a = F.tlo[0] + (int)(t % F.tn[0]), b = F.tlo[1] + (int)(t / F.tn[0]);
    bool ok;
    switch (2 * F.dir + F.side) {
    case 0: ok = hse_column<0, false>(U, T, P, a, b); break;
    case 1: ok = hse_column<0, true>(U, T, P, a, b); break;
    case 2: ok = hse_column<1, false>(U, T, P, a, b); break;
    case 3: ok = hse_column<1, true>(U, T, P, a, b); break;
    default: ok = hse_column<2, false>(U, T, P, a, b); break;       // no hydrostatic fill above +z (hse_fill.cpp:986-993)
    }
    if (!ok && unconverged) atomicAdd(unconverged, 1);
}

} // namespace

int launch_ext_bc_fill(const DFab& U, const int flo[3], const int fhi[3], const ::castro_amd_geom* geom, const DevParams& P,
                       const ::castro_amd_ext_bc* ext, int* d_unconverged, hipStream_t stream, Profiler* prof)
{
    if (geom->coord != 0) return CASTRO_AMD_ERR_UNSUPPORTED;
    // external boundaries meeting at an edge (Castro_bc_fill_nd.cpp:74-100); opposite faces are fine
    bool inflow[3];
    for (int d = 0; d < 3; ++d) inflow[d] = geom->lo_bc[d] == BC_INFLOW || geom->hi_bc[d] == BC_INFLOW;
    if ((int)inflow[0] + (int)inflow[1] + (int)inflow[2] > 1) return CASTRO_AMD_ERR_UNSUPPORTED;
    if (geom->hi_bc[2] == BC_INFLOW && ext->hi_type[2] == EXT_HSE) return CASTRO_AMD_ERR_UNSUPPORTED;
    // a FAB without a zone of the domain has nothing to start from
    for (int d = 0; d < 3; ++d) if (fhi[d] < geom->domlo[d] || flo[d] > geom->domhi[d]) return CASTRO_AMD_OK;

    // the HSE faces the FAB reaches across, and what their walks read inside the domain
    HseDev T;
    T.nface = 0; T.ntot = 0;
    T.zero_vels = ext->hse_zero_vels; T.interp_temp = ext->hse_interp_temp; T.reflect_vels = ext->hse_reflect_vels;
    T.const_grav = ext->const_grav;
    for (int d = 0; d < 3; ++d) {
        T.dx[d] = geom->dx[d]; T.domlo[d] = geom->domlo[d]; T.domhi[d] = geom->domhi[d]; T.flo[d] = flo[d]; T.fhi[d] = fhi[d];
    }
    for (int d = 0; d < 3; ++d)
        for (int side = 0; side < 2; ++side) {
            const bool hse = side == 0 ? (geom->lo_bc[d] == BC_INFLOW && ext->lo_type[d] == EXT_HSE)
                                       : (geom->hi_bc[d] == BC_INFLOW && ext->hi_type[d] == EXT_HSE);
            if (!hse) continue;
            if (ext->hse_interp_temp == 1 && geom->domhi[d] - geom->domlo[d] + 1 < 2) return CASTRO_AMD_ERR_ARG;
            const int nghost = side == 0 ? geom->domlo[d] - flo[d] : fhi[d] - geom->domhi[d];
            if (nghost <= 0) continue;
            const int ninside = side == 0 ? (fhi[d] < geom->domhi[d] ? fhi[d] : geom->domhi[d]) - geom->domlo[d] + 1
                                          : geom->domhi[d] - (flo[d] > geom->domlo[d] ? flo[d] : geom->domlo[d]) + 1;
            if (ext->hse_interp_temp == 1 && ninside < 2) return CASTRO_AMD_ERR_ARG;
            if (ext->hse_zero_vels != 1 && ext->hse_reflect_vels == 1 && ninside < nghost) return CASTRO_AMD_ERR_ARG;
            HseFace& F = T.f[T.nface++];
            F.dir = d; F.side = side;
            const int t0 = d == 0 ? 1 : 0, t1 = d == 2 ? 1 : 2;
            F.tlo[0] = flo[t0]; F.tn[0] = fhi[t0] - flo[t0] + 1;
            F.tlo[1] = flo[t1]; F.tn[1] = fhi[t1] - flo[t1] + 1;
            F.start = T.ntot;
            T.ntot += (long)F.tn[0] * F.tn[1];
        }

    if (ext->fill_ambient_bc == 1) {
        AmbDev A;
        int blo[3], bhi[3];
        for (int d = 0; d < 3; ++d) {
            const bool dir_on = ext->ambient_fill_dir == d || ext->ambient_fill_dir == -1;
            A.domlo[d] = geom->domlo[d]; A.domhi[d] = geom->domhi[d];
            A.amb_lo[d] = dir_on && geom->lo_bc[d] == BC_OUTFLOW;
            A.amb_hi[d] = dir_on && geom->hi_bc[d] == BC_OUTFLOW;
            blo[d] = (A.amb_lo[d] && flo[d] < geom->domlo[d]) ? geom->domlo[d] : flo[d];
            bhi[d] = (A.amb_hi[d] && fhi[d] > geom->domhi[d]) ? geom->domhi[d] : fhi[d];
        }
        A.outflow_vel = ext->ambient_outflow_vel;
        for (int n = 0; n < NUM_STATE; ++n) A.state[n] = ext->ambient_state[n];
        const Slabs S = shell_slabs(flo, fhi, blo, bhi);        // the zones beyond an ambient face
        if (S.start[6] > 0) {
            const dim3 grid((unsigned)((S.start[6] + 255) / 256));
            for (int branch = (A.outflow_vel == 1 ? 0 : -1); branch < (A.outflow_vel == 1 ? 3 : 0); ++branch) {
                prof_begin(prof, "k_ambient_fill", stream);
                hipLaunchKernelGGL(k_ambient_fill, grid, dim3(256), 0, stream, U, S, A, branch);
                prof_end(prof, stream);
            }
        }
    }
    if (T.ntot > 0) {
        prof_begin(prof, "k_hse_fill", stream);
        hipLaunchKernelGGL(k_hse_fill, dim3((unsigned)((T.ntot + 255) / 256)), dim3(256), 0, stream, U, T, P, d_unconverged);
        prof_end(prof, stream);
    }
    return hipGetLastError() == hipSuccess ? CASTRO_AMD_OK : CASTRO_AMD_ERR_HIP;
}

} // namespace cad

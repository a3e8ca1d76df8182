// ctu_kernels.hip -- the CTU hydro advance as HIP kernels for gfx950 (MI355X).
//
// Pipeline for one tile bx (replaces the 75 ParallelFor launches of
// Source/hydro/Castro_ctu_hydro.cpp:130-1480):
//
//   k_ctoprim      U(Sborder) -> compact primitives Q = (rho,u,v,w,p,rhoe,X,c)     [ctoprim + EOS]
//   k_divu         Q -> node-centred div(u) (+ shock flag for the hybrid solver)   [divu, shock]
//   k_trace_pair   Q -> flattening coefficient (registers only) -> PPM parabolas ->
//                  characteristic tracing in x,y,z -> edge states QM/QP, and the first
//                  x Riemann solve on the faces between lanes -> F1[x]             [uflatten + 3x trace_ppm + cmpflx]
//                  (k_trace<SRC,PLM>: one zone per thread, with old_source / PLM;
//                   k_riemann1_blockstart: the x faces at workgroup starts)
//   k_riemann1<D>  QM/QP[D] -> first transverse fluxes F1[D] (+ Godunov un, p)     [cmpflx_plus_godunov, D = y, z]
//   k_trans1       QM/QP[N] + F1[T1], F1[T2] -> corrected states (registers only)
//                  -> Riemann -> F2[N|T1], F2[N|T2], N = x, y, z in one launch     [6x trans_single (x2) + 6x cmpflx]
//   k_final<N>     QM/QP[N] + F2[T1|T2], F2[T2|T1] -> ql,qr (registers) -> Riemann ->
//                  artificial viscosity, species normalisation, scaling,
//                  fluxes += / = , mass_fluxes = , qe                              [trans_final, cmpflx, apply_av,
//                                                                                   normalize_species_fluxes, scale_flux]
//   k_consup       S_new (+)= dt*div(F) - dt*p*div(u) term, optionally followed in
//                  registers by S_new.min, clean_state and the CFL estimate          [consup_hydro (+ clean_state, estdt_cfl)]
//
// The heavy kernels process two x-adjacent zones (faces) per thread with 16-byte accesses; a caller may split
// the update into the part that reads no ghost zone and the rest (CASTRO_AMD_STAGE_A / _B, launch_ctu_hydro).
//
// Data layout.  All scratch arrays share ONE index space: the tile grown by 4 (same as
// Sborder), unit stride along x, one plane of NC doubles per component (SoA), so every
// load/store of a wavefront is a contiguous 512-byte run along the x pencil.
//
// Addressing.  Every access is `uniform plane base (SGPR pair) + 32-bit byte offset
// (one VGPR)`: the global_load/store "saddr" form.  A thread carries ONE offset for its
// zone in the scratch space and one for its zone in each caller FAB; neighbours are
// offset +- stride.  (64-bit per-access pointers cost two VGPRs and a v_lshl_add_u64 each.)
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "hydro_device.h"
#include "ctu_kernels.h"

// the Colella-Glaz instantiations (GEN == 2) carry the out-of-line NaN-sign fall-back (hydro_device.h: XD), whose call
// frame would push them past 256 VGPRs to one wave per SIMD; held at two waves the overflow is spilled around the call only
// (Sedov 256^3, riemann_solver = 1: k_trans1 18.6 -> see DESIGN.md section 9)
#if !defined(CG_ONE_WAVE)
#ifndef FINAL_MIN_WAVES         // A/B (round 6, profiles/r06f_*): 3 = the fold / final / update kernels held to 168 registers for a third wave
#define FINAL_MIN_WAVES 1
#endif
#define CG_TWO_WAVES __attribute__((amdgpu_waves_per_eu(GEN == 2 ? 2 : FINAL_MIN_WAVES, GEN == 2 ? 2 : 8)))
#else
#define CG_TWO_WAVES
#endif
namespace cad {

// Host-free stepping: DevParams::dtp points at castro_amd_step_control's vector; once a step has been rejected
// (ctl[CASTRO_AMD_CTL_STATUS] != 0) the launches that follow in the same batch must leave the caller's arrays alone --
// the host retries from the old state of the rejected step.
#define RETURN_IF_BATCH_FAILED() if (P.dtp && P.dtp[3] != 0.0) return

// ---------------------------------------------------------------------------------------
// addressing helpers
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double ldg(const double* base, unsigned boff)
{
    return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + boff);
}
__device__ __forceinline__ void stg(double* base, unsigned boff, double v)
{
#ifndef PLAIN_STORES            // non-temporal stores: what a kernel writes is not read again before it has left every cache,
                                // so it should not evict the stencil neighbours from L2 (step -4 %, k_trace -12 %)
    __builtin_nontemporal_store(v, reinterpret_cast<double*>(reinterpret_cast<char*>(base) + boff));
#else
    *reinterpret_cast<double*>(reinterpret_cast<char*>(base) + boff) = v;
#endif
}

// Two x-adjacent zones per thread.  The stencil kernels issue ~100 vector-memory instructions per
// zone and are bound by the rate at which a CU can issue them (TA busy 70-90 %, tools/ta_bench.hip),
// not by bytes: a 16-byte access moves two zones per instruction.  8-byte alignment is enough
// (unaligned 16-byte global accesses run at full rate on gfx950, same benchmark).
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));
struct D2 { double a, b; };
__device__ __forceinline__ D2 ldg2(const double* base, unsigned boff)
{
#ifdef EXPERIMENT_NT_LOADS
    const d2u v = __builtin_nontemporal_load(reinterpret_cast<const d2u*>(reinterpret_cast<const char*>(base) + boff));
#else
    const d2u v = *reinterpret_cast<const d2u*>(reinterpret_cast<const char*>(base) + boff);
#endif
    return D2{ v.x, v.y };
}
__device__ __forceinline__ void stg2(double* base, unsigned boff, double a, double b)
{
    d2u v; v.x = a; v.y = b;
#ifndef PLAIN_STORES
    __builtin_nontemporal_store(v, reinterpret_cast<d2u*>(reinterpret_cast<char*>(base) + boff));
#else
    *reinterpret_cast<d2u*>(reinterpret_cast<char*>(base) + boff) = v;
#endif
}

// byte offset of zone (i,j,k) in the scratch index space / in a caller FAB
__device__ __forceinline__ unsigned goff(const Tile& t, int i, int j, int k)
{
    return 8u * ((unsigned)(i - t.glo[0]) + (unsigned)t.NX * ((unsigned)(j - t.glo[1]) + (unsigned)t.NY * (unsigned)(k - t.glo[2])));
}
__device__ __forceinline__ unsigned foff(const DFab& f, int i, int j, int k)
{
    return 8u * ((unsigned)(i - f.lo[0]) + (unsigned)f.sy * ((unsigned)(j - f.lo[1])) + (unsigned)f.sz * (unsigned)(k - f.lo[2]));
}
// byte strides of the scratch space
struct Str { unsigned x, y, z; };
__device__ __forceinline__ Str gstr(const Tile& t) { return Str{ 8u, 8u * (unsigned)t.NX, 8u * (unsigned)t.NX * (unsigned)t.NY }; }
__device__ __forceinline__ unsigned dstr(const Str& s, int d) { return d == 0 ? s.x : d == 1 ? s.y : s.z; }

// one zone (or face) per thread, x fastest over the whole box: a wavefront touches one contiguous
// 512-byte run per array plane.  (Brick-shaped workgroups, XCD-contiguous workgroup ids and
// marching workgroups were all measured slower on MI355X: DESIGN.md "Launch shape".)
// `ty` > 0 selects the XCD-tiled order: workgroup ids are dealt round-robin to the 8 XCDs by the
// dispatcher, so id -> (id % 8) * (nb / 8) + id / 8 hands each XCD one contiguous run of rows, and
// the rows are enumerated y-tile by y-tile (ty rows), z-plane by z-plane inside a tile, so that the
// workgroups resident on one XCD at a time share their y and z stencil neighbours through that XCD's L2.
struct LinBox { int lo[3], n[3]; int ty; unsigned nb; int w, hi0; unsigned wg; };   // w zones per thread along x (n[0] counts threads); wg threads per workgroup

__device__ __forceinline__ bool box_thread_at(const LinBox& b, unsigned bid, unsigned thr, int& i, int& j, int& k)
{
    if (b.ty > 0) {
        const unsigned per = b.nb >> 3;          // nb is a multiple of 8 in this mode
        bid = (bid & 7u) * per + (bid >> 3);
    }
    const unsigned tid = bid * b.wg + thr;
    const unsigned total = (unsigned)b.n[0] * (unsigned)b.n[1] * (unsigned)b.n[2];
    if (tid >= total) return false;
    const unsigned ii = tid % (unsigned)b.n[0];
    const unsigned r = tid / (unsigned)b.n[0];
    i = b.lo[0] + b.w * (int)ii;
    if (b.ty > 0) {
        const unsigned rpt = (unsigned)b.ty * (unsigned)b.n[2];
        const unsigned yt = r / rpt;
        const unsigned rem = r - yt * rpt;
        const unsigned left = (unsigned)b.n[1] - yt * (unsigned)b.ty;
        const unsigned tyh = left < (unsigned)b.ty ? left : (unsigned)b.ty;
        const unsigned kk = rem / tyh;
        j = b.lo[1] + (int)(yt * (unsigned)b.ty + (rem - kk * tyh));
        k = b.lo[2] + (int)kk;
    } else {
        j = b.lo[1] + (int)(r % (unsigned)b.n[1]);
        k = b.lo[2] + (int)(r / (unsigned)b.n[1]);
    }
    return true;
}

__device__ __forceinline__ bool box_thread(const LinBox& b, int& i, int& j, int& k)
{
    return box_thread_at(b, blockIdx.x, threadIdx.x, i, j, k);
}

// ---------------------------------------------------------------------------------------
// A whole level in one launch (castro_amd_ctu_hydro_mf, round 4).  The kernels of the default path take an optional box
// table: workgroup ids are then cut into per-box ranges by a prefix array (every range a multiple of 8 workgroups, so the
// round-robin XCD dealing that LinBox::ty relies on holds inside each range), and the per-box arguments -- tile, launch
// geometry, scratch and caller arrays -- come from the table instead of the kernel arguments.  A level of 56 boxes of ~45^3
// zones is then 8 launches that fill the chip instead of ~450 that each fill a fraction of it.
// ---------------------------------------------------------------------------------------
struct XRows { int lo[3]; int hi0; int nslot, ny, nz; int ty; unsigned nb; unsigned wv; };   // k_finalx_consup; wv: waves per workgroup
enum : int { LB_CTOPRIM = 0, LB_DIVU = 1, LB_TRACE = 2, LB_FOLD = 3, LB_FY = 4, LB_FZ = 5, LB_FX = 6, LB_BSTART = 7,
             LB_SRCPRIM = 8, LB_TRACE1 = 9, LB_R1X = 10, NLB = 11 };     // 8 .. 10: a level with traced source terms (round 6)
struct LevelBox {
    Tile t;
    DevScratch S;
    DFab U, Unew, fl[3], mass[3], qe[3];
    int acc_hi[3];
    LinBox b[6];           // LB_CTOPRIM .. LB_FZ
    XRows xr;              // LB_FX
    DFab Src;              // the old-time source FAB of the box (p == nullptr: none)
    LinBox bs[3];          // LB_SRCPRIM (grow(bx, 3), one zone per thread), LB_TRACE1 (grow(bx, 1), one zone per thread), LB_R1X (x faces, pairs)
};
struct LevelTab { const LevelBox* box; const unsigned* start; int nbox; };   // start: nbox + 1 entries of THIS launch; box == nullptr: one box, kernel arguments

// the box a workgroup belongs to; vb becomes its id inside that box's range
__device__ __forceinline__ const LevelBox& level_box(const LevelTab& lv, unsigned& vb)
{
    int lo = 0, hi = lv.nbox;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (lv.start[mid] <= vb) lo = mid; else hi = mid;
    }
    vb -= lv.start[lo];
    return lv.box[lo];
}

// ---------------------------------------------------------------------------------------
// Castro::ctoprim (Source/hydro/advection_util.cpp:26-200) with the gamma-law EOS inlined
// ---------------------------------------------------------------------------------------
// zones inside [lo,hi] are left to another launch (staged execution, see launch_ctu_hydro); empty = none
struct SkipBox { int lo[3], hi[3]; };
__device__ __forceinline__ bool in_skip(const SkipBox& s, int i, int j, int k)
{
    return i >= s.lo[0] && i <= s.hi[0] && j >= s.lo[1] && j <= s.hi[1] && k >= s.lo[2] && k <= s.hi[2];
}

// CLEAN: Castro::clean_state applied `clean_n` times to the zone first, in place (castro_amd_hydro_opts.sborder_clean_ntimes):
// the clean_state(S_old) of initialize_advance and the clean_state(Sborder) after FillPatch inside the pass that reads the
// state anyway.  Plain stores: k_final / k_finalx_consup read the cleaned zones again.
// Up to six boxes in one launch, x fastest inside each (the ghost shell of a box as z, y and x slabs): thread -> zone
struct ShellBoxes { int lo[6][3], nn[6][3]; unsigned start[7]; };
__device__ __forceinline__ bool shell_thread(const ShellBoxes& S, int& i, int& j, int& k)
{
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= S.start[6]) return false;
    int r = 0;
    while (tid >= S.start[r + 1]) ++r;
    const unsigned q = tid - S.start[r];
    const unsigned n0 = (unsigned)S.nn[r][0], n1 = (unsigned)S.nn[r][1];
    i = S.lo[r][0] + (int)(q % n0);
    const unsigned rr = q / n0;
    j = S.lo[r][1] + (int)(rr % n1);
    k = S.lo[r][2] + (int)(rr / n1);
    return true;
}
struct BcKinds { int lo[3], hi[3]; int kind_lo[3], kind_hi[3]; };   // domain extent; kind 0 leave (interior / periodic), 1 extrapolate, 2 mirror

// One zone of k_ctoprim.  `bc`: the zone (i,j,k) lies outside the problem domain in a non-periodic direction and takes the state of
// the in-domain zone (si,sj,sk) -- the physical-boundary part of FillPatch (Source/problems/Castro_bc_fill_nd.cpp:11-125; BC tables
// Castro_setup.cpp:40-53: clamp to the nearest interior zone for outflow / inflow (FOEXTRAP), mirror about the boundary with the
// normal momentum negated for symmetry and walls (REFLECT_ODD: fx, fy, fz)) fused with ctoprim: the source zone has been cleaned by
// an earlier launch already (clean_state commutes with the copy and with the mirror image: it is zone-local and even in the
// momenta), so the copy is stored into Sborder as it is (the artificial viscosity of the final stage reads one ghost layer of it),
// the clean_state loop below runs zero times, and the primitive record follows from the SAME instructions as for every other
// zone of this kernel -- boundary zones, ghost-shell zones and valid zones share one compiled copy of the arithmetic, so the
// `contract` build (whose FMA contraction may differ between two copies of one expression) gives the bits of
// k_bc_fill + k_ctoprim whatever the launch partition.
template <bool CLEAN>
__device__ __forceinline__ void ctoprim_zone(const Tile& t, const DFab& U, double* __restrict__ Q, const DevParams& P, int* status,
                                             int clean_n, int lean_q, int i, int j, int k,
                                             int si, int sj, int sk, bool fx, bool fy, bool fz, bool bc)
{
    // lean_q (gamma_law_edges, default-solver path of the `contract` build), bit 0: nobody downstream reads Q's (rho e) and X
    // planes; bit 1: the update kernel has clean_state fused in and reads neither the temperature nor the species of U
    const unsigned c = goff(t, i, j, k);
    const unsigned cd = foff(U, i, j, k);           // where the zone lives
    const unsigned cu = foff(U, si, sj, sk);        // where its state is read from (== cd unless bc)
    const long NC = t.NC;

    double rho = ldg(U.p + URHO * U.sn, cu);
    double mx = ldg(U.p + UMX * U.sn, cu), my = ldg(U.p + UMY * U.sn, cu), mz = ldg(U.p + UMZ * U.sn, cu);
    double eden = ldg(U.p + UEDEN * U.sn, cu);
    if (fx) mx = -mx;                               // norm_vel_bc: REFLECT_ODD
    if (fy) my = -my;
    if (fz) mz = -mz;
    // lean_q: with one species and a gamma-law gas nothing downstream reads the temperature or the species of this array
    // (X is elided, the fused update recomputes both: k_finalx_consup), so they are neither loaded, cleaned nor written back
    const bool lean_u = (lean_q & 2) != 0;
    double rX = lean_u ? rho : ldg(U.p + UFS * U.sn, cu);
    double eint = 0.0;
    double* up = U.p;
    if (bc) {
        // the boundary fill proper: all eight components of the source zone, whatever this build reads of them
        eint = ldg(U.p + UEINT * U.sn, cu);
        const double tb = ldg(U.p + UTEMP * U.sn, cu), xb = ldg(U.p + UFS * U.sn, cu);
#define PUT(comp, v) *reinterpret_cast<double*>(reinterpret_cast<char*>(up + (comp) * U.sn) + cd) = (v)
        PUT(URHO, rho); PUT(UMX, mx); PUT(UMY, my); PUT(UMZ, mz); PUT(UEDEN, eden); PUT(UEINT, eint); PUT(UTEMP, tb); PUT(UFS, xb);
#undef PUT
    }
    if (CLEAN) {
        if (!bc) eint = ldg(U.p + UEINT * U.sn, cu);
        double temp = lean_u ? 0.0 : ldg(U.p + UTEMP * U.sn, cu);
        const double o0 = rho, o1 = mx, o2 = my, o3 = mz, o4 = eden, o5 = eint, o6 = temp, o7 = rX;
        clean_zone(P, clean_n, rho, mx, my, mz, eden, eint, temp, rX);          // clean_n == 0 in a boundary zone
        // Only components whose bits changed go back: the state arrives cleaned twice by the update that produced it, and
        // the applications here almost always reproduce it (8 planes less to write; a plane nobody changes stays clean in L2).
#define PUT_IF_CHANGED(comp, o, v) \
        if (__double_as_longlong(o) != __double_as_longlong(v)) *reinterpret_cast<double*>(reinterpret_cast<char*>(up + (comp) * U.sn) + cd) = (v)
        PUT_IF_CHANGED(URHO, o0, rho);
        PUT_IF_CHANGED(UMX, o1, mx);
        PUT_IF_CHANGED(UMY, o2, my);
        PUT_IF_CHANGED(UMZ, o3, mz);
        PUT_IF_CHANGED(UEDEN, o4, eden);
        PUT_IF_CHANGED(UEINT, o5, eint);
        if (!lean_u) {
            PUT_IF_CHANGED(UTEMP, o6, temp);
            PUT_IF_CHANGED(UFS, o7, rX);
        }
#undef PUT_IF_CHANGED
    }
    if (rho <= 0.0 || rho < P.small_dens) atomicOr(status, 1);

    const double rhoinv = frcp(rho);               // rho >= small_dens > 0 (else the status flag above is raised)
    const double u = mx * rhoinv;
    const double v = my * rhoinv;
    const double w = mz * rhoinv;

    const double kineng = 0.5 * rho * (u * u + v * v + w * w);

    double e;
    if ((eden - kineng) > P.eta1 * eden) {
        e = (eden - kineng) * rhoinv;
    } else {
        e = ((CLEAN || bc) ? eint : ldg(U.p + UEINT * U.sn, cu)) * rhoinv;
    }

    const double X = rX * rhoinv;

    // eos(eos_input_re): p = (gamma-1) rho e ; cs = sqrt(gamma p / rho)
    const double p = (P.gamma - 1.0) * rho * e;
    const double cs = kContract ? fsqrt(P.gamma * p * rhoinv) : sqrt(P.gamma * p / rho);

    stg(Q + PRHO * NC, c, rho);
    stg(Q + PU * NC, c, u);
    stg(Q + PV * NC, c, v);
    stg(Q + PW * NC, c, w);
    stg(Q + PP * NC, c, p);
    if (!(lean_q & 1)) {
        stg(Q + PRE * NC, c, e * rho);
        stg(Q + PX * NC, c, X);
    }
    stg(Q + PC * NC, c, cs);
}

// mode 0: the zones of the LinBox `b` (minus `skip`); 1: the zones of the boxes `sh` (the ghost shell of a box whose valid zones an
// earlier launch has done: CASTRO_AMD_STAGE_REST, ONE launch for the six slabs); 2: the zones of `sh` as physical-boundary zones
// (CASTRO_AMD_BC_FILL: source zone by the per-direction index map of M, see ctoprim_zone).  One kernel for the three, so that
// every zone goes through the same compiled arithmetic.
template <bool CLEAN, bool LV = false>
__global__ void __launch_bounds__(256) k_ctoprim(Tile t, LinBox b, DFab U, double* __restrict__ Q, DevParams P, int* status,
                                                 SkipBox skip, int clean_n, LevelTab lv, int lean_q, int mode, ShellBoxes sh, BcKinds M)
{
    RETURN_IF_BATCH_FAILED();
    int ijk[3], s[3];
    bool flip[3] = { false, false, false };
    if (LV || mode == 0) {
        unsigned vb = blockIdx.x;
        if (LV) { const LevelBox& B = level_box(lv, vb); t = B.t; b = B.b[LB_CTOPRIM]; U = B.U; Q = B.S.Q; }
        if (!box_thread_at(b, vb, threadIdx.x, ijk[0], ijk[1], ijk[2])) return;
        if (in_skip(skip, ijk[0], ijk[1], ijk[2])) return;
    } else {
        if (!shell_thread(sh, ijk[0], ijk[1], ijk[2])) return;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) s[d] = ijk[d];
    const bool bc = !LV && mode == 2;
    if (bc) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (ijk[d] < M.lo[d] && M.kind_lo[d] != 0) {
                if (M.kind_lo[d] == 1) s[d] = M.lo[d];
                else { s[d] = 2 * M.lo[d] - ijk[d] - 1; flip[d] = true; }
            } else if (ijk[d] > M.hi[d] && M.kind_hi[d] != 0) {
                if (M.kind_hi[d] == 1) s[d] = M.hi[d];
                else { s[d] = 2 * M.hi[d] - ijk[d] + 1; flip[d] = true; }
            }
        }
    }
    ctoprim_zone<CLEAN>(t, U, Q, P, status, bc ? 0 : clean_n, lean_q, ijk[0], ijk[1], ijk[2], s[0], s[1], s[2], flip[0], flip[1], flip[2], bc);
}

// ---------------------------------------------------------------------------------------
// Castro::src_to_prim (Source/hydro/Castro_ctu.cpp:468-545) on grow(bx,3): conserved old-time
// sources -> primitive sources (CTU, source_term_predictor = 0: srcU = old_source)
// ---------------------------------------------------------------------------------------
// CORR (p != nullptr with source_term_predictor = 1): Castro::source_corrector, dt/2 of it time-centres the momentum sources
// lean (gamma_law_edges): Q carries no (rho e) plane -- it is p / (gamma - 1) -- and nobody reads the (rho e) source plane
template <bool LV = false>
__global__ void __launch_bounds__(256) k_src_to_prim(Tile t, LinBox b, const double* __restrict__ Q, DFab SRC,
                                                     double* __restrict__ SQ, DevParams P, DFab CORR, double dt, int lean, LevelTab lv)
{
    unsigned vb = blockIdx.x;
    // LV: every box of a level in one launch (round 6: levels with traced source terms) -- tile, launch box, planes and source FAB from the table
    if (LV) { const LevelBox& B = level_box(lv, vb); t = B.t; b = B.bs[0]; Q = B.S.Q; SRC = B.Src; SQ = B.S.SRCQ; }
    int i, j, k;
    if (!box_thread_at(b, vb, threadIdx.x, i, j, k)) return;
    if (P.dtp) dt = P.dtp[6];
    const unsigned c = goff(t, i, j, k);
    const unsigned cs = foff(SRC, i, j, k);
    const long NC = t.NC;

    const double s_rho = 0.0 + ldg(SRC.p + URHO * SRC.sn, cs);
    double s_mx = 0.0, s_my = 0.0, s_mz = 0.0;
    if (CORR.p) {                                  // Castro_ctu.cpp:493-497
        const unsigned cc = foff(CORR, i, j, k);
        s_mx += 0.5 * dt * ldg(CORR.p + UMX * CORR.sn, cc);
        s_my += 0.5 * dt * ldg(CORR.p + UMY * CORR.sn, cc);
        s_mz += 0.5 * dt * ldg(CORR.p + UMZ * CORR.sn, cc);
    }
    s_mx += ldg(SRC.p + UMX * SRC.sn, cs);
    s_my += ldg(SRC.p + UMY * SRC.sn, cs);
    s_mz += ldg(SRC.p + UMZ * SRC.sn, cs);
    const double s_ei = 0.0 + ldg(SRC.p + UEINT * SRC.sn, cs);

    const double rho = ldg(Q + PRHO * NC, c);
    const double rhoinv = 1.0 / rho;
    const double qre = lean ? ldg(Q + PP * NC, c) * (1.0 / (P.gamma - 1.0)) : ldg(Q + PRE * NC, c);
    const double e = qre * rhoinv;
    const double dpde = (P.gamma - 1.0) * rho;
    const double dpdr_e = (P.gamma - 1.0) * e;

    const double q_rho = s_rho;
    stg(SQ + PRHO * NC, c, q_rho);
    stg(SQ + PU * NC, c, (s_mx - ldg(Q + PU * NC, c) * q_rho) * rhoinv);
    stg(SQ + PV * NC, c, (s_my - ldg(Q + PV * NC, c) * q_rho) * rhoinv);
    stg(SQ + PW * NC, c, (s_mz - ldg(Q + PW * NC, c) * q_rho) * rhoinv);
    if (!lean) stg(SQ + PRE * NC, c, s_ei);
    stg(SQ + PP * NC, c, dpde * (s_ei - qre * q_rho * rhoinv) * rhoinv + dpdr_e * q_rho);
}

// ---------------------------------------------------------------------------------------
// Castro::divu, 3-D branch (Source/hydro/advection_util.cpp:458-475), nodes of grow(bx,1)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_divu(Tile t, LinBox b, const double* __restrict__ Q, double* __restrict__ DIV,
                                              double* __restrict__ SHK, double dxinv, double dyinv, double dzinv)
{
    int i, j, k;
    if (!box_thread(b, i, j, k)) return;
    const unsigned c = goff(t, i, j, k);
    const Str s = gstr(t);
    const unsigned sx = s.x, sy = s.y, sz = s.z;
    const double* QU_ = Q + PU * t.NC;
    const double* QV_ = Q + PV * t.NC;
    const double* QW_ = Q + PW * t.NC;

    double ux = 0.25 * (ldg(QU_, c) - ldg(QU_, c - sx) +
                        ldg(QU_, c - sz) - ldg(QU_, c - sx - sz) +
                        ldg(QU_, c - sy) - ldg(QU_, c - sx - sy) +
                        ldg(QU_, c - sy - sz) - ldg(QU_, c - sx - sy - sz)) * dxinv;

    double vy = 0.25 * (ldg(QV_, c) - ldg(QV_, c - sy) +
                        ldg(QV_, c - sz) - ldg(QV_, c - sy - sz) +
                        ldg(QV_, c - sx) - ldg(QV_, c - sx - sy) +
                        ldg(QV_, c - sx - sz) - ldg(QV_, c - sx - sy - sz)) * dyinv;

    double wz = 0.25 * (ldg(QW_, c) - ldg(QW_, c - sz) +
                        ldg(QW_, c - sy) - ldg(QW_, c - sy - sz) +
                        ldg(QW_, c - sx) - ldg(QW_, c - sx - sz) +
                        ldg(QW_, c - sx - sy) - ldg(QW_, c - sx - sy - sz)) * dzinv;

    stg(DIV, c, ux + vy + wz);

    // Castro::shock (Source/hydro/advection_util.cpp:203-363), 3-D Cartesian: only needed by the
    // hybrid Riemann solver (Castro_ctu_hydro.cpp:294-303); the default zero-fill is elided
    if (SHK) {
        constexpr double small = 1.e-10;
        constexpr double eps = 0.33e0;
        const double* QP_ = Q + PP * t.NC;
        double div_u = 0.0;
        div_u += 0.5 * (ldg(QU_, c + sx) - ldg(QU_, c - sx)) * dxinv;
        div_u += 0.5 * (ldg(QV_, c + sy) - ldg(QV_, c - sy)) * dyinv;
        div_u += 0.5 * (ldg(QW_, c + sz) - ldg(QW_, c - sz)) * dzinv;

        double px_pre, px_post, py_pre, py_post, pz_pre, pz_post;
        if (ldg(QP_, c + sx) - ldg(QP_, c - sx) < 0.0) { px_pre = ldg(QP_, c + sx); px_post = ldg(QP_, c - sx); }
        else { px_pre = ldg(QP_, c - sx); px_post = ldg(QP_, c + sx); }
        double e_x = (ldg(QU_, c + sx) - ldg(QU_, c - sx)) * (ldg(QU_, c + sx) - ldg(QU_, c - sx));

        if (ldg(QP_, c + sy) - ldg(QP_, c - sy) < 0.0) { py_pre = ldg(QP_, c + sy); py_post = ldg(QP_, c - sy); }
        else { py_pre = ldg(QP_, c - sy); py_post = ldg(QP_, c + sy); }
        double e_y = (ldg(QV_, c + sy) - ldg(QV_, c - sy)) * (ldg(QV_, c + sy) - ldg(QV_, c - sy));

        if (ldg(QP_, c + sz) - ldg(QP_, c - sz) < 0.0) { pz_pre = ldg(QP_, c + sz); pz_post = ldg(QP_, c - sz); }
        else { pz_pre = ldg(QP_, c - sz); pz_post = ldg(QP_, c + sz); }
        double e_z = (ldg(QW_, c + sz) - ldg(QW_, c - sz)) * (ldg(QW_, c + sz) - ldg(QW_, c - sz));

        double denom = 1.0 / (e_x + e_y + e_z + small);
        e_x = e_x * denom;
        e_y = e_y * denom;
        e_z = e_z * denom;

        double p_pre = e_x * px_pre + e_y * py_pre + e_z * pz_pre;
        double p_post = e_x * px_post + e_y * py_post + e_z * pz_post;

        double pjump = (p_pre == 0) ? 0.0 : eps - (p_post - p_pre) / p_pre;

        stg(SHK, c, (pjump < 0.0 && div_u < 0.0) ? 1.0 : 0.0);
    }
}

// the same for two x-adjacent nodes per thread (no shock flag): per velocity plane and row one 16-byte load of the
// zones (i, i+1) and one 8-byte load of zone i-1 instead of four 8-byte loads
// div(u) at the nodes (i, j, k) and (i+1, j, k) -- the low corners of the thread's two zones; shared by k_divu_pair and by
// k_trace_pair, which computes it in front of its own work where the launch covers the same box (round 6: one launch less)
__device__ __forceinline__ void divu_pair_body(const Tile& t, const double* __restrict__ Q, double* __restrict__ DIV, unsigned c, bool v1,
                                               double dxinv, double dyinv, double dzinv)
{
    const Str s = gstr(t);
    const unsigned sx = s.x, sy = s.y, sz = s.z;
    const double* QU_ = Q + PU * t.NC;
    const double* QV_ = Q + PV * t.NC;
    const double* QW_ = Q + PW * t.NC;
    // a[r] = zone i-1, m[r] = zones (i, i+1) of row r: 0 (j,k), 1 (j,k-1), 2 (j-1,k), 3 (j-1,k-1)
    const unsigned ro[4] = { 0u, sz, sy, sy + sz };
    double ua[4], va[4], wa[4];
    D2 um[4], vm[4], wm[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        um[r] = ldg2(QU_, c - ro[r]); ua[r] = ldg(QU_, c - ro[r] - sx);
        vm[r] = ldg2(QV_, c - ro[r]); va[r] = ldg(QV_, c - ro[r] - sx);
        wm[r] = ldg2(QW_, c - ro[r]); wa[r] = ldg(QW_, c - ro[r] - sx);
    }
    double d[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        // hi = zone of the node's own column, lo = the column to its left
#define HI(x, r) (w ? x##m[r].b : x##m[r].a)
#define LO(x, r) (w ? x##m[r].a : x##a[r])
        double ux = 0.25 * (HI(u, 0) - LO(u, 0) + HI(u, 1) - LO(u, 1) + HI(u, 2) - LO(u, 2) + HI(u, 3) - LO(u, 3)) * dxinv;
        double vy = 0.25 * (HI(v, 0) - HI(v, 2) + HI(v, 1) - HI(v, 3) + LO(v, 0) - LO(v, 2) + LO(v, 1) - LO(v, 3)) * dyinv;
        double wz = 0.25 * (HI(w, 0) - HI(w, 1) + HI(w, 2) - HI(w, 3) + LO(w, 0) - LO(w, 1) + LO(w, 2) - LO(w, 3)) * dzinv;
#undef HI
#undef LO
        d[w] = ux + vy + wz;
    }
    if (v1) stg2(DIV, c, d[0], d[1]);
    else stg(DIV, c, d[0]);
}

template <bool LV = false>
__global__ void __launch_bounds__(256) k_divu_pair(Tile t, LinBox b, const double* __restrict__ Q, double* __restrict__ DIV,
                                                   double dxinv, double dyinv, double dzinv, LevelTab lv)
{
    unsigned vb = blockIdx.x;
    if (LV) { const LevelBox& B = level_box(lv, vb); t = B.t; b = B.b[LB_DIVU]; Q = B.S.Q; DIV = B.S.DIV; }
    int i, j, k;
    if (!box_thread_at(b, vb, threadIdx.x, i, j, k)) return;
    divu_pair_body(t, Q, DIV, goff(t, i, j, k), i + 1 <= b.hi0, dxinv, dyinv, dzinv);
}

// ---------------------------------------------------------------------------------------
// flattening + PPM + tracing.  Castro::uflatten (flatten.cpp:12-166) and Castro::trace_ppm
// (trace_ppm.cpp:15-594, no sources) for the three directions of one zone of grow(bx,1).
// ---------------------------------------------------------------------------------------
// one source component: trace under it only if its 5-point stencil is not identically zero
// (check_trace_source, ppm.H:11-41 -- the reference's GPU form; the CPU form pre-scans the
// tile, trace_ppm.cpp:66-93, and gives the same numbers because an all-zero stencil integrates
// to exactly zero)
template <int NW>
__device__ __forceinline__ void trace_source(const double* __restrict__ a, unsigned c, unsigned sd, double flat,
                                             double un, double cc, double dtdx, double Ip[3], double Im[3])
{
    double s[5];
    s[0] = ldg(a, c - 2 * sd); s[1] = ldg(a, c - sd); s[2] = ldg(a, c); s[3] = ldg(a, c + sd); s[4] = ldg(a, c + 2 * sd);
    Ip[0] = Ip[1] = Ip[2] = 0.0;
    Im[0] = Im[1] = Im[2] = 0.0;
    const bool do_trace = fabs(s[0]) > 0.0 || fabs(s[1]) > 0.0 || fabs(s[2]) > 0.0 || fabs(s[3]) > 0.0 || fabs(s[4]) > 0.0;
    if (do_trace) {
        double sm, sp;
        ppm_reconstruct(s, flat, sm, sp);
        const double s6 = 6.0 * s[2] - 3.0 * (sm + sp);
        if (NW == 3) {            // rho, p, rho e: all three waves
            ppm_int_wave(sm, sp, s6, un - cc, dtdx, Ip[0], Im[0]);
            ppm_int_wave(sm, sp, s6, un, dtdx, Ip[1], Im[1]);
            ppm_int_wave(sm, sp, s6, un + cc, dtdx, Ip[2], Im[2]);
        } else if (NW == 2) {     // normal velocity: u-c and u+c
            ppm_int_wave(sm, sp, s6, un - cc, dtdx, Ip[0], Im[0]);
            ppm_int_wave(sm, sp, s6, un + cc, dtdx, Ip[2], Im[2]);
        } else {                  // transverse velocities: contact only
            ppm_int_wave(sm, sp, s6, un, dtdx, Ip[1], Im[1]);
        }
    }
}

// GL (gamma_law_edges, see trace_finish): the (rho e) and X variables are neither loaded, traced nor stored.  With source terms
// the identity still holds: for a gamma-law gas src_to_prim's p source is (gamma - 1) times its (rho e) source
// (dpde (s_e - e s_rho) / rho ... + dpdr_e s_rho = (gamma - 1) s_e, Castro_ctu.cpp:525-540), so the traced (rho e) -- parabola
// integrals plus dt/2 times the source integrals, all linear -- is the traced p over (gamma - 1); X has no source.
template <int D, bool SRC, bool GL = false>
__device__ __forceinline__ void trace_dir(const Tile& t, const double* __restrict__ Q, const double* __restrict__ SQ,
                                          unsigned c, unsigned sd,
                                          double flat, double dtdx, double hdt, const DevParams& P,
                                          bool do_plus, bool do_minus,
                                          double* __restrict__ QMd, double* __restrict__ QPd)
{
    // trace_ppm.cpp:114-128
    constexpr int QUN = (D == 0) ? PU : (D == 1) ? PV : PW;
    constexpr int QUT = (D == 0) ? PV : (D == 1) ? PW : PU;
    constexpr int QUTT = (D == 0) ? PW : (D == 1) ? PU : PV;

    const long NC = t.NC;
    const double cc = ldg(Q + PC * NC, c);
    const double un = ldg(Q + QUN * NC, c);

    double s[5], sm, sp, s6;

#define LOAD5(comp) { const double* a = Q + (long)(comp) * NC; \
        s[0] = ldg(a, c - 2 * sd); s[1] = ldg(a, c - sd); s[2] = ldg(a, c); s[3] = ldg(a, c + sd); s[4] = ldg(a, c + 2 * sd); }

    // density: three waves
    double Ip_rho0, Im_rho0, Ip_rho1, Im_rho1, Ip_rho2, Im_rho2;
    LOAD5(PRHO);
    ppm_reconstruct(s, flat, sm, sp);
    s6 = 6.0 * s[2] - 3.0 * (sm + sp);
    ppm_int_wave(sm, sp, s6, un - cc, dtdx, Ip_rho0, Im_rho0);
    ppm_int_wave(sm, sp, s6, un, dtdx, Ip_rho1, Im_rho1);
    ppm_int_wave(sm, sp, s6, un + cc, dtdx, Ip_rho2, Im_rho2);

    // normal velocity: u-c and u+c
    double Ip_un_0, Im_un_0, Ip_un_2, Im_un_2;
    LOAD5(QUN);
    ppm_reconstruct(s, flat, sm, sp);
    s6 = 6.0 * s[2] - 3.0 * (sm + sp);
    ppm_int_wave(sm, sp, s6, un - cc, dtdx, Ip_un_0, Im_un_0);
    ppm_int_wave(sm, sp, s6, un + cc, dtdx, Ip_un_2, Im_un_2);

    // pressure: three waves
    double Ip_p0, Im_p0, Ip_p1, Im_p1, Ip_p2, Im_p2;
    LOAD5(PP);
    ppm_reconstruct(s, flat, sm, sp);
    s6 = 6.0 * s[2] - 3.0 * (sm + sp);
    ppm_int_wave(sm, sp, s6, un - cc, dtdx, Ip_p0, Im_p0);
    ppm_int_wave(sm, sp, s6, un, dtdx, Ip_p1, Im_p1);
    ppm_int_wave(sm, sp, s6, un + cc, dtdx, Ip_p2, Im_p2);

    // rho e: three waves
    double Ip_re0 = 0.0, Im_re0 = 0.0, Ip_re1 = 0.0, Im_re1 = 0.0, Ip_re2 = 0.0, Im_re2 = 0.0;
    if (!GL) {
    LOAD5(PRE);
    ppm_reconstruct(s, flat, sm, sp);
    s6 = 6.0 * s[2] - 3.0 * (sm + sp);
    ppm_int_wave(sm, sp, s6, un - cc, dtdx, Ip_re0, Im_re0);
    ppm_int_wave(sm, sp, s6, un, dtdx, Ip_re1, Im_re1);
    ppm_int_wave(sm, sp, s6, un + cc, dtdx, Ip_re2, Im_re2);
    }

    // transverse velocities and the passive: contact wave only
    double Ip_ut, Im_ut, Ip_utt, Im_utt, Ip_X, Im_X;
    LOAD5(QUT);
    ppm_reconstruct(s, flat, sm, sp);
    s6 = 6.0 * s[2] - 3.0 * (sm + sp);
    ppm_int_wave(sm, sp, s6, un, dtdx, Ip_ut, Im_ut);

    LOAD5(QUTT);
    ppm_reconstruct(s, flat, sm, sp);
    s6 = 6.0 * s[2] - 3.0 * (sm + sp);
    ppm_int_wave(sm, sp, s6, un, dtdx, Ip_utt, Im_utt);

    if (!GL) {
    LOAD5(PX);
    ppm_reconstruct(s, flat, sm, sp);
    s6 = 6.0 * s[2] - 3.0 * (sm + sp);
    ppm_int_wave(sm, sp, s6, un, dtdx, Ip_X, Im_X);
    } else { Ip_X = Im_X = 1.0; }
#undef LOAD5

    // source terms (trace_ppm.cpp:226-330); SQ planes are indexed like the primitive components
    double Ips_rho[3], Ims_rho[3], Ips_un[3], Ims_un[3], Ips_p[3], Ims_p[3], Ips_re[3], Ims_re[3];
    double Ips_ut[3], Ims_ut[3], Ips_utt[3], Ims_utt[3];
    if (SRC) {
        trace_source<3>(SQ + PRHO * NC, c, sd, flat, un, cc, dtdx, Ips_rho, Ims_rho);
        trace_source<2>(SQ + (long)QUN * NC, c, sd, flat, un, cc, dtdx, Ips_un, Ims_un);
        trace_source<3>(SQ + PP * NC, c, sd, flat, un, cc, dtdx, Ips_p, Ims_p);
        if (!GL) trace_source<3>(SQ + PRE * NC, c, sd, flat, un, cc, dtdx, Ips_re, Ims_re);
        else { Ips_re[0] = Ips_re[1] = Ips_re[2] = Ims_re[0] = Ims_re[1] = Ims_re[2] = 0.0; }
        trace_source<1>(SQ + (long)QUT * NC, c, sd, flat, un, cc, dtdx, Ips_ut, Ims_ut);
        trace_source<1>(SQ + (long)QUTT * NC, c, sd, flat, un, cc, dtdx, Ips_utt, Ims_utt);
    }
#define SADD(x, sv) (SRC ? ((x) + hdt * (sv)) : (x))
#define SSUB(x, sv) (SRC ? ((x) - hdt * (sv)) : (x))

    // gamma_c is the constant eos_gamma for a gamma-law gas: its parabola is flat and
    // Ip = Im = gamma exactly (sm == sp == s0 => quadratic limiter resets, s6 == 0), so the
    // reference's QGAMC reconstruction (trace_ppm.cpp:212-223) is elided bit-for-bit.
    const double gam = P.gamma;

    if (do_plus) {
        // plus state on face i, trace_ppm.cpp:382-466 (source integrals are zero)
        double rho_ref = SADD(Im_rho0, Ims_rho[0]);
        double un_ref = SADD(Im_un_0, Ims_un[0]);
        double p_ref = SADD(Im_p0, Ims_p[0]);
        double rhoe_g_ref = SADD(Im_re0, Ims_re[0]);

        // rho_ref >= small_dens, p_ref >= small_pres: every operand of the fast forms is a normal number far from the range ends
        rho_ref = amax(rho_ref, P.small_dens);
        double rho_ref_inv = frcp(rho_ref);
        p_ref = amax(p_ref, P.small_pres);

        double csq_ref = gam * p_ref * rho_ref_inv;
        double cc_ref = fsqrt(csq_ref);
        double cc_ref_inv = frcp(cc_ref);
        double h_g_ref = (p_ref + rhoe_g_ref) * rho_ref_inv;

        double dum = SSUB(un_ref - Im_un_0, Ims_un[0]);
        double dptotm = SSUB(p_ref - Im_p0, Ims_p[0]);

        double drho = SSUB(rho_ref - Im_rho1, Ims_rho[1]);
        double dptot = SSUB(p_ref - Im_p1, Ims_p[1]);
        double drhoe_g = SSUB(rhoe_g_ref - Im_re1, Ims_re[1]);

        double dup = SSUB(un_ref - Im_un_2, Ims_un[2]);
        double dptotp = SSUB(p_ref - Im_p2, Ims_p[2]);

        double alpham = 0.5 * (dptotm * rho_ref_inv * cc_ref_inv - dum) * rho_ref * cc_ref_inv;
        double alphap = 0.5 * (dptotp * rho_ref_inv * cc_ref_inv + dup) * rho_ref * cc_ref_inv;
        double alpha0r, alpha0e_g;
        if (kContract) {
            const double csq_inv = cc_ref_inv * cc_ref_inv;
            alpha0r = drho - dptot * csq_inv;
            alpha0e_g = drhoe_g - dptot * h_g_ref * csq_inv;
        } else {
            alpha0r = drho - dptot / csq_ref;
            alpha0e_g = drhoe_g - dptot * h_g_ref / csq_ref;
        }

        alpham = un - cc > 0.0 ? 0.0 : -alpham;
        alphap = un + cc > 0.0 ? 0.0 : -alphap;
        alpha0r = un > 0.0 ? 0.0 : -alpha0r;
        alpha0e_g = un > 0.0 ? 0.0 : -alpha0e_g;

        stg(QPd + PRHO * NC, c, amax(P.small_dens, rho_ref + alphap + alpham + alpha0r));
        stg(QPd + QUN * NC, c, un_ref + (alphap - alpham) * cc_ref * rho_ref_inv);
        if (!GL) stg(QPd + PRE * NC, c, amax(P.small_dens_ener, rhoe_g_ref + (alphap + alpham) * h_g_ref + alpha0e_g));
        stg(QPd + PP * NC, c, amax(P.small_pres, p_ref + (alphap + alpham) * csq_ref));
        stg(QPd + QUT * NC, c, SADD(Im_ut, Ims_ut[1]));
        stg(QPd + QUTT * NC, c, SADD(Im_utt, Ims_utt[1]));
        if (!GL) stg(QPd + PX * NC, c, Im_X);
    }

    if (do_minus) {
        // minus state on face i+1, trace_ppm.cpp:470-561
        double rho_ref = SADD(Ip_rho2, Ips_rho[2]);
        double un_ref = SADD(Ip_un_2, Ips_un[2]);
        double p_ref = SADD(Ip_p2, Ips_p[2]);
        double rhoe_g_ref = SADD(Ip_re2, Ips_re[2]);

        // rho_ref >= small_dens, p_ref >= small_pres: every operand of the fast forms is a normal number far from the range ends
        rho_ref = amax(rho_ref, P.small_dens);
        double rho_ref_inv = frcp(rho_ref);
        p_ref = amax(p_ref, P.small_pres);

        double csq_ref = gam * p_ref * rho_ref_inv;
        double cc_ref = fsqrt(csq_ref);
        double cc_ref_inv = frcp(cc_ref);
        double h_g_ref = (p_ref + rhoe_g_ref) * rho_ref_inv;

        double dum = SSUB(un_ref - Ip_un_0, Ips_un[0]);
        double dptotm = SSUB(p_ref - Ip_p0, Ips_p[0]);

        double drho = SSUB(rho_ref - Ip_rho1, Ips_rho[1]);
        double dptot = SSUB(p_ref - Ip_p1, Ips_p[1]);
        double drhoe_g = SSUB(rhoe_g_ref - Ip_re1, Ips_re[1]);

        double dup = SSUB(un_ref - Ip_un_2, Ips_un[2]);
        double dptotp = SSUB(p_ref - Ip_p2, Ips_p[2]);

        double alpham = 0.5 * (dptotm * rho_ref_inv * cc_ref_inv - dum) * rho_ref * cc_ref_inv;
        double alphap = 0.5 * (dptotp * rho_ref_inv * cc_ref_inv + dup) * rho_ref * cc_ref_inv;
        double alpha0r, alpha0e_g;
        if (kContract) {
            const double csq_inv = cc_ref_inv * cc_ref_inv;
            alpha0r = drho - dptot * csq_inv;
            alpha0e_g = drhoe_g - dptot * h_g_ref * csq_inv;
        } else {
            alpha0r = drho - dptot / csq_ref;
            alpha0e_g = drhoe_g - dptot * h_g_ref / csq_ref;
        }

        alpham = un - cc > 0.0 ? -alpham : 0.0;
        alphap = un + cc > 0.0 ? -alphap : 0.0;
        alpha0r = un > 0.0 ? -alpha0r : 0.0;
        alpha0e_g = un > 0.0 ? -alpha0e_g : 0.0;

        const unsigned cp = c + sd;
        stg(QMd + PRHO * NC, cp, amax(P.small_dens, rho_ref + alphap + alpham + alpha0r));
        stg(QMd + QUN * NC, cp, un_ref + (alphap - alpham) * cc_ref * rho_ref_inv);
        if (!GL) stg(QMd + PRE * NC, cp, amax(P.small_dens_ener, rhoe_g_ref + (alphap + alpham) * h_g_ref + alpha0e_g));
        stg(QMd + PP * NC, cp, amax(P.small_pres, p_ref + (alphap + alpham) * csq_ref));
        stg(QMd + QUT * NC, cp, SADD(Ip_ut, Ips_ut[1]));
        stg(QMd + QUTT * NC, cp, SADD(Ip_utt, Ips_utt[1]));
        if (!GL) stg(QMd + PX * NC, cp, Ip_X);
    }
#undef SADD
#undef SSUB
}


// ---------------------------------------------------------------------------------------
// PPM tracing without source terms, two x-adjacent zones per thread (the benchmark path).
// Same arithmetic as trace_dir<D, false>: the stencils of both zones come from shared 16-byte loads.
// ---------------------------------------------------------------------------------------
struct TraceW {        // parabola integrals under the u-c, u, u+c waves for one zone and one direction
    double Ip_rho[3], Im_rho[3], Ip_un[3], Im_un[3], Ip_p[3], Im_p[3], Ip_re[3], Im_re[3];
    double Ip_ut[3], Im_ut[3], Ip_utt[3], Im_utt[3], Ip_X[3], Im_X[3];   // [1] only
};

template <int NW>
__device__ __forceinline__ void ppm_waves(const double s[5], double flat, double un, double cc, double dtdx,
                                          double Ip[3], double Im[3])
{
    double sm, sp;
    ppm_reconstruct(s, flat, sm, sp);
    const double s6 = 6.0 * s[2] - 3.0 * (sm + sp);
    if (NW == 3) {
        ppm_int_wave(sm, sp, s6, un - cc, dtdx, Ip[0], Im[0]);
        ppm_int_wave(sm, sp, s6, un, dtdx, Ip[1], Im[1]);
        ppm_int_wave(sm, sp, s6, un + cc, dtdx, Ip[2], Im[2]);
    } else if (NW == 2) {
        ppm_int_wave(sm, sp, s6, un - cc, dtdx, Ip[0], Im[0]);
        ppm_int_wave(sm, sp, s6, un + cc, dtdx, Ip[2], Im[2]);
    } else {
        ppm_int_wave(sm, sp, s6, un, dtdx, Ip[1], Im[1]);
    }
}

// characteristic projection of trace_ppm.cpp:382-561 with zero source integrals
// GL (the `contract` build's default-solver path): gamma-law shortcut.  With (rho e) = p / (gamma - 1) in every zone -- what
// ctoprim hands over for this EOS -- the parabolas of (rho e) are those of p divided by (gamma - 1) (the limiters are invariant
// under a positive scaling), h_g_ref / csq_ref = 1 / (gamma - 1), alpha0e_g vanishes identically and the traced (rho e) is the
// traced p over (gamma - 1).  So the (rho e) stencils are neither loaded nor reconstructed and the edge state's (rho e) is not
// stored: every reader of QM / QP takes it from p (load_edge_2<NOPRE>).  Exact in real arithmetic away from the small_pres
// floor; a rounding away from the reference's expression, hence `contract` only.
//
// The same switch elides the species.  This build has ONE species (NumSpec = 1), and for one species the
// reference's own last word on the species flux is normalize_species_fluxes (advection_util.cpp:577-613): F[UFS] = F[UFS] *
// (F[URHO] / F[UFS]) = F[URHO], whatever the traced, transversally corrected and upwinded X was (unless the interface X is
// below 2e-16, which normalize_species excludes for a cleaned state).  X is passive -- nothing else reads it -- so every
// operation on it from the PPM parabola to the Riemann upwinding is dead with respect to the outputs: the GEN == 0 kernels of the
// `contract` build neither trace, store, load nor correct X (edge states: 5 planes instead of 7; state-form records: 6
// instead of 7; FL: 8 instead of 9) and set F[UFS] = F[URHO] where the reference normalises.  One rounding away from the
// reference (its F[UFS] is F[URHO] (1 +- 2 ulp)).
__host__ __device__ constexpr bool gamma_law_edges(int GEN)
{
#ifdef CAD_NUMERICS_CONTRACT
    return GEN == 0;
#else
    return (void)GEN, false;
#endif
}

template <int D, bool GL = false>
__device__ __forceinline__ void trace_finish(const TraceW& w, double un, double cc, const DevParams& P,
                                             double qp[NEDGE], double qm[NEDGE])
{
    constexpr int QUN = (D == 0) ? PU : (D == 1) ? PV : PW;
    constexpr int QUT = (D == 0) ? PV : (D == 1) ? PW : PU;
    constexpr int QUTT = (D == 0) ? PW : (D == 1) ? PU : PV;
    const double gam = P.gamma;
    {
        // plus state on face i, trace_ppm.cpp:382-466
        double rho_ref = w.Im_rho[0];
        double un_ref = w.Im_un[0];
        double p_ref = w.Im_p[0];
        double rhoe_g_ref = GL ? 0.0 : w.Im_re[0];

        // rho_ref >= small_dens, p_ref >= small_pres: every operand of the fast forms is a normal number far from the range ends
        rho_ref = amax_cu(rho_ref, P.small_dens);
        double rho_ref_inv = frcp(rho_ref);
        p_ref = amax_cu(p_ref, P.small_pres);

        double csq_ref = gam * p_ref * rho_ref_inv;
        double cc_ref = fsqrt(csq_ref);
        double cc_ref_inv = frcp(cc_ref);
        double h_g_ref = (p_ref + rhoe_g_ref) * rho_ref_inv;

        double dum = un_ref - w.Im_un[0];
        double dptotm = p_ref - w.Im_p[0];

        double drho = rho_ref - w.Im_rho[1];
        double dptot = p_ref - w.Im_p[1];
        double drhoe_g = GL ? 0.0 : rhoe_g_ref - w.Im_re[1];

        double dup = un_ref - w.Im_un[2];
        double dptotp = p_ref - w.Im_p[2];

        double alpham = 0.5 * (dptotm * rho_ref_inv * cc_ref_inv - dum) * rho_ref * cc_ref_inv;
        double alphap = 0.5 * (dptotp * rho_ref_inv * cc_ref_inv + dup) * rho_ref * cc_ref_inv;
        double alpha0r, alpha0e_g;
        if (kContract) {
            const double csq_inv = cc_ref_inv * cc_ref_inv;
            alpha0r = drho - dptot * csq_inv;
            alpha0e_g = drhoe_g - dptot * h_g_ref * csq_inv;
        } else {
            alpha0r = drho - dptot / csq_ref;
            alpha0e_g = drhoe_g - dptot * h_g_ref / csq_ref;
        }

        alpham = un - cc > 0.0 ? 0.0 : -alpham;
        alphap = un + cc > 0.0 ? 0.0 : -alphap;
        alpha0r = un > 0.0 ? 0.0 : -alpha0r;
        alpha0e_g = un > 0.0 ? 0.0 : -alpha0e_g;

        qp[PRHO] = amax_hw(P.small_dens, rho_ref + alphap + alpham + alpha0r);      // positive parameter first (hydro_device.h)
        qp[QUN] = un_ref + (alphap - alpham) * cc_ref * rho_ref_inv;
        qp[PP] = amax_hw(P.small_pres, p_ref + (alphap + alpham) * csq_ref);
        qp[PRE] = GL ? qp[PP] * (1.0 / (gam - 1.0)) : amax_hw(P.small_dens_ener, rhoe_g_ref + (alphap + alpham) * h_g_ref + alpha0e_g);
        qp[QUT] = w.Im_ut[1];
        qp[QUTT] = w.Im_utt[1];
        qp[PX] = w.Im_X[1];
    }
    {
        // minus state on face i+1, trace_ppm.cpp:470-561
        double rho_ref = w.Ip_rho[2];
        double un_ref = w.Ip_un[2];
        double p_ref = w.Ip_p[2];
        double rhoe_g_ref = GL ? 0.0 : w.Ip_re[2];

        // rho_ref >= small_dens, p_ref >= small_pres: every operand of the fast forms is a normal number far from the range ends
        rho_ref = amax_cu(rho_ref, P.small_dens);
        double rho_ref_inv = frcp(rho_ref);
        p_ref = amax_cu(p_ref, P.small_pres);

        double csq_ref = gam * p_ref * rho_ref_inv;
        double cc_ref = fsqrt(csq_ref);
        double cc_ref_inv = frcp(cc_ref);
        double h_g_ref = (p_ref + rhoe_g_ref) * rho_ref_inv;

        double dum = un_ref - w.Ip_un[0];
        double dptotm = p_ref - w.Ip_p[0];

        double drho = rho_ref - w.Ip_rho[1];
        double dptot = p_ref - w.Ip_p[1];
        double drhoe_g = GL ? 0.0 : rhoe_g_ref - w.Ip_re[1];

        double dup = un_ref - w.Ip_un[2];
        double dptotp = p_ref - w.Ip_p[2];

        double alpham = 0.5 * (dptotm * rho_ref_inv * cc_ref_inv - dum) * rho_ref * cc_ref_inv;
        double alphap = 0.5 * (dptotp * rho_ref_inv * cc_ref_inv + dup) * rho_ref * cc_ref_inv;
        double alpha0r, alpha0e_g;
        if (kContract) {
            const double csq_inv = cc_ref_inv * cc_ref_inv;
            alpha0r = drho - dptot * csq_inv;
            alpha0e_g = drhoe_g - dptot * h_g_ref * csq_inv;
        } else {
            alpha0r = drho - dptot / csq_ref;
            alpha0e_g = drhoe_g - dptot * h_g_ref / csq_ref;
        }

        alpham = un - cc > 0.0 ? -alpham : 0.0;
        alphap = un + cc > 0.0 ? -alphap : 0.0;
        alpha0r = un > 0.0 ? -alpha0r : 0.0;
        alpha0e_g = un > 0.0 ? -alpha0e_g : 0.0;

        qm[PRHO] = amax_hw(P.small_dens, rho_ref + alphap + alpham + alpha0r);
        qm[QUN] = un_ref + (alphap - alpham) * cc_ref * rho_ref_inv;
        qm[PP] = amax_hw(P.small_pres, p_ref + (alphap + alpham) * csq_ref);
        qm[PRE] = GL ? qm[PP] * (1.0 / (gam - 1.0)) : amax_hw(P.small_dens_ener, rhoe_g_ref + (alphap + alpham) * h_g_ref + alpha0e_g);
        qm[QUT] = w.Ip_ut[1];
        qm[QUTT] = w.Ip_utt[1];
        qm[PX] = w.Ip_X[1];
    }
}

template <bool NOPRE = false>          // NOPRE: the (rho e) and X planes are not stored (gamma_law_edges)
__device__ __forceinline__ void store_edge_2(double* __restrict__ E, long NC, unsigned c, const double q[2][NEDGE], bool m0, bool m1)
{
#ifdef TRACE_DIAG_NOSTORE     // timing diagnostic (wrong results): the edge-state stores behind a condition that never holds
    if (q[0][PRHO] != 1.2345e300) return;
#endif
    if (m0 && m1) {
#pragma unroll
        for (int n = 0; n < NEDGE; ++n) { if (NOPRE && (n == PRE || n == PX)) continue; stg2(E + (long)n * NC, c, q[0][n], q[1][n]); }
    } else if (m0) {
#pragma unroll
        for (int n = 0; n < NEDGE; ++n) { if (NOPRE && (n == PRE || n == PX)) continue; stg(E + (long)n * NC, c, q[0][n]); }
    } else if (m1) {
#pragma unroll
        for (int n = 0; n < NEDGE; ++n) { if (NOPRE && (n == PRE || n == PX)) continue; stg(E + (long)n * NC, c + 8u, q[1][n]); }
    }
}

// five-point stencils of two x-adjacent zones along direction D
template <int D>
__device__ __forceinline__ void load_stencil_2(const double* __restrict__ a, unsigned c, unsigned sd, double sA[5], double sB[5])
{
    if (D == 0) {
        const D2 l = ldg2(a, c - 16u), m = ldg2(a, c), r = ldg2(a, c + 16u);
        sA[0] = l.a; sA[1] = l.b; sA[2] = m.a; sA[3] = m.b; sA[4] = r.a;
        sB[0] = l.b; sB[1] = m.a; sB[2] = m.b; sB[3] = r.a; sB[4] = r.b;
    } else {
#ifdef TRACE_DIAG_CENTER_ONLY      // timing diagnostic (wrong results): one load per y / z stencil instead of five
        const D2 v = ldg2(a, c);
#pragma unroll
        for (int m = -2; m <= 2; ++m) { sA[m + 2] = v.a * (1.0 + 0.01 * m); sB[m + 2] = v.b * (1.0 - 0.01 * m); }
        (void)sd;
#else
#pragma unroll
        for (int m = -2; m <= 2; ++m) { const D2 v = ldg2(a, c + m * sd); sA[m + 2] = v.a; sB[m + 2] = v.b; }
#endif
    }
}

// aA/aB enter holding the stencils of the normal velocity, bA/bB those of the density; with NEXT >= 0 they leave
// holding the density (a) and normal-velocity (b) stencils of direction NEXT (stride sdn), requested before the
// characteristic projection and the stores of this direction.
// GL (gamma_law_edges): the (rho e) and X variables are skipped (the two stencil buffers still change roles an odd number of
// times: the routine leaves with a = density, b = normal velocity of direction NEXT like the full form).
template <int D, int NEXT, bool GL = false>
__device__ __forceinline__ void trace_pair_dir(const Tile& t, const double* __restrict__ Q, unsigned c, unsigned sd, unsigned sdn,
                                               const double flat[2], double dtdx, const DevParams& P,
                                               const bool do_plus[2], const bool do_minus[2],
                                               double* __restrict__ QMd, double* __restrict__ QPd,
                                               double qp[2][NEDGE], double qm[2][NEDGE],
                                               double aA[5], double aB[5], double bA[5], double bB[5])
{
    constexpr int QUN = (D == 0) ? PU : (D == 1) ? PV : PW;
    constexpr int QUT = (D == 0) ? PV : (D == 1) ? PW : PU;
    constexpr int QUTT = (D == 0) ? PW : (D == 1) ? PU : PV;
    const long NC = t.NC;
    const D2 ccv = ldg2(Q + PC * NC, c);
    const double cc[2] = { ccv.a, ccv.b };

    TraceW w[2];
    double un[2];
    // software pipeline: the stencil of the next variable is requested before the parabola of the current one
    // is evaluated (two register buffers): 3.30 -> 3.16 ms at 256^3
    un[0] = aA[2]; un[1] = aB[2];
    ppm_waves<2>(aA, flat[0], un[0], cc[0], dtdx, w[0].Ip_un, w[0].Im_un);
    ppm_waves<2>(aB, flat[1], un[1], cc[1], dtdx, w[1].Ip_un, w[1].Im_un);

    load_stencil_2<D>(Q + (long)PP * NC, c, sd, aA, aB);
    ppm_waves<3>(bA, flat[0], un[0], cc[0], dtdx, w[0].Ip_rho, w[0].Im_rho);
    ppm_waves<3>(bB, flat[1], un[1], cc[1], dtdx, w[1].Ip_rho, w[1].Im_rho);

    if (GL) {
        load_stencil_2<D>(Q + (long)QUT * NC, c, sd, bA, bB);
        ppm_waves<3>(aA, flat[0], un[0], cc[0], dtdx, w[0].Ip_p, w[0].Im_p);
        ppm_waves<3>(aB, flat[1], un[1], cc[1], dtdx, w[1].Ip_p, w[1].Im_p);

        load_stencil_2<D>(Q + (long)QUTT * NC, c, sd, aA, aB);
        ppm_waves<1>(bA, flat[0], un[0], cc[0], dtdx, w[0].Ip_ut, w[0].Im_ut);
        ppm_waves<1>(bB, flat[1], un[1], cc[1], dtdx, w[1].Ip_ut, w[1].Im_ut);

        // no parabola for X either (see gamma_law_edges): two variables fewer, the buffers leave in the usual roles
        if (NEXT >= 0) load_stencil_2<(NEXT >= 0 ? NEXT : 0)>(Q + (long)(NEXT == 1 ? PV : PW) * NC, c, sdn, bA, bB);
        ppm_waves<1>(aA, flat[0], un[0], cc[0], dtdx, w[0].Ip_utt, w[0].Im_utt);
        ppm_waves<1>(aB, flat[1], un[1], cc[1], dtdx, w[1].Ip_utt, w[1].Im_utt);
        if (NEXT >= 0) load_stencil_2<(NEXT >= 0 ? NEXT : 0)>(Q + (long)PRHO * NC, c, sdn, aA, aB);
        w[0].Ip_X[1] = w[0].Im_X[1] = w[1].Ip_X[1] = w[1].Im_X[1] = 1.0;

        trace_finish<D, true>(w[0], un[0], cc[0], P, qp[0], qm[0]);
        trace_finish<D, true>(w[1], un[1], cc[1], P, qp[1], qm[1]);

#ifdef TRACE_DIAG_STORES_AT_END       // timing diagnostic (wrong results): the x and y edge states are not stored where they are computed ...
        if (D == 2)
#endif
        {
        store_edge_2<true>(QPd, NC, c, qp, do_plus[0], do_plus[1]);
        store_edge_2<true>(QMd, NC, c + sd, qm, do_minus[0], do_minus[1]);
        }
        return;
    }
    load_stencil_2<D>(Q + (long)PRE * NC, c, sd, bA, bB);
    ppm_waves<3>(aA, flat[0], un[0], cc[0], dtdx, w[0].Ip_p, w[0].Im_p);
    ppm_waves<3>(aB, flat[1], un[1], cc[1], dtdx, w[1].Ip_p, w[1].Im_p);

    load_stencil_2<D>(Q + (long)QUT * NC, c, sd, aA, aB);
    ppm_waves<3>(bA, flat[0], un[0], cc[0], dtdx, w[0].Ip_re, w[0].Im_re);
    ppm_waves<3>(bB, flat[1], un[1], cc[1], dtdx, w[1].Ip_re, w[1].Im_re);

    load_stencil_2<D>(Q + (long)QUTT * NC, c, sd, bA, bB);
    ppm_waves<1>(aA, flat[0], un[0], cc[0], dtdx, w[0].Ip_ut, w[0].Im_ut);
    ppm_waves<1>(aB, flat[1], un[1], cc[1], dtdx, w[1].Ip_ut, w[1].Im_ut);

    load_stencil_2<D>(Q + (long)PX * NC, c, sd, aA, aB);
    ppm_waves<1>(bA, flat[0], un[0], cc[0], dtdx, w[0].Ip_utt, w[0].Im_utt);
    ppm_waves<1>(bB, flat[1], un[1], cc[1], dtdx, w[1].Ip_utt, w[1].Im_utt);

    if (NEXT >= 0) load_stencil_2<(NEXT >= 0 ? NEXT : 0)>(Q + (long)(NEXT == 1 ? PV : PW) * NC, c, sdn, bA, bB);
    ppm_waves<1>(aA, flat[0], un[0], cc[0], dtdx, w[0].Ip_X, w[0].Im_X);
    ppm_waves<1>(aB, flat[1], un[1], cc[1], dtdx, w[1].Ip_X, w[1].Im_X);
    if (NEXT >= 0) load_stencil_2<(NEXT >= 0 ? NEXT : 0)>(Q + (long)PRHO * NC, c, sdn, aA, aB);

    trace_finish<D>(w[0], un[0], cc[0], P, qp[0], qm[0]);
    trace_finish<D>(w[1], un[1], cc[1], P, qp[1], qm[1]);

    store_edge_2(QPd, NC, c, qp, do_plus[0], do_plus[1]);
    store_edge_2(QMd, NC, c + sd, qm, do_minus[0], do_minus[1]);
}

// ---------------------------------------------------------------------------------------
// PLM characteristic tracing (ppm_type = 0), Castro::trace_plm, trace_plm.cpp:17-339, fused with the
// reflecting-boundary fix-up of Castro::ctu_plm_states (Castro_ctu.cpp:287-433): at a Symmetry
// face the zone inside the domain writes both edge states and the ghost zone writes neither.
// ---------------------------------------------------------------------------------------
// GL (the `contract` build's default-solver path, round 6): the gamma-law shortcut of trace_finish for the PLM trace.  With (rho e) =
// p / (gamma - 1) in every zone the limited slope of (rho e) is that of p over (gamma - 1) (every limiter of uslope is invariant under a
// positive scaling; castro.use_pslope = 1 changes the slope of p alone and is excluded by the launcher), enth = 1 / (gamma - 1), alpha0e
// vanishes and the traced (rho e) is the traced p over (gamma - 1): neither loaded, traced nor stored -- and neither is the one species.
template <int D, bool SRC, bool GL = false>
__device__ __forceinline__ void trace_plm_dir(const Tile& t, const double* __restrict__ Q, const double* __restrict__ SQ,
                                              unsigned c, unsigned sd, int idx, const DevGeom& g,
                                              double flat, double dt, const DevParams& P,
                                              bool do_plus, bool do_minus,
                                              double* __restrict__ QMd, double* __restrict__ QPd)
{
    constexpr int QUN = (D == 0) ? PU : (D == 1) ? PV : PW;
    constexpr int QUT = (D == 0) ? PV : (D == 1) ? PW : PU;
    constexpr int QUTT = (D == 0) ? PW : (D == 1) ? PU : PV;

    const long NC = t.NC;
    const double dtdx = dt / g.dx[D];
    const bool lo_bc_test = g.sym_lo[D] && idx == g.domlo[D];
    const bool hi_bc_test = g.sym_hi[D] && idx == g.domhi[D];
    // ghost zones just outside a Symmetry face leave that face to the zone inside
    if (g.sym_lo[D] && idx == g.domlo[D] - 1) do_minus = false;
    if (g.sym_hi[D] && idx == g.domhi[D] + 1) do_plus = false;

#define LOAD5(arr, comp, dst) { const double* a = (arr) + (long)(comp) * NC; \
        dst[0] = ldg(a, c - 2 * sd); dst[1] = ldg(a, c - sd); dst[2] = ldg(a, c); dst[3] = ldg(a, c + sd); dst[4] = ldg(a, c + 2 * sd); }

    double srho[5], sp[5], s[5];
    LOAD5(Q, PRHO, srho);
    LOAD5(Q, PP, sp);

    const double cc = ldg(Q + PC * NC, c);
    const double csq = cc * cc;
    const double rho = srho[2];
    const double p = sp[2];
    const double enth_rhoe = GL ? 0.0 : ldg(Q + PRE * NC, c);

    const double dq_rho = uslope(srho, flat, false, false, P);
    LOAD5(Q, QUN, s);
    const double un = s[2];
    const double dq_un = uslope(s, flat, lo_bc_test, hi_bc_test, P);
    LOAD5(Q, QUT, s);
    const double ut = s[2];
    const double dq_ut = uslope(s, flat, false, false, P);
    LOAD5(Q, QUTT, s);
    const double utt = s[2];
    const double dq_utt = uslope(s, flat, false, false, P);
    double dq_p = uslope(sp, flat, false, false, P);
    double rhoe = 0.0, dq_re = 0.0, X = 1.0, dX = 0.0, enth = 0.0;
    if (!GL) {
        LOAD5(Q, PRE, s);
        rhoe = enth_rhoe;
        dq_re = uslope(s, flat, false, false, P);
        LOAD5(Q, PX, s);
        X = s[2];
        dX = uslope(s, flat, false, false, P);

        enth = (rhoe + p) / (rho * csq);
    }

    if (P.use_pslope == 1) {
        double src[5];
        if (SRC) { LOAD5(SQ, QUN, src); }
        else { src[0] = src[1] = src[2] = src[3] = src[4] = 0.0; }
        pslope(srho, sp, src, flat, lo_bc_test, hi_bc_test, g.dx[D], dq_p, P);
    }
#undef LOAD5

    // old-time sources at the zone centre (zero planes when the caller passes no source)
    double sq_rho = 0.0, sq_un = 0.0, sq_ut = 0.0, sq_utt = 0.0, sq_p = 0.0, sq_re = 0.0;
    if (SRC) {
        sq_rho = ldg(SQ + PRHO * NC, c);
        sq_un = ldg(SQ + (long)QUN * NC, c);
        sq_ut = ldg(SQ + (long)QUT * NC, c);
        sq_utt = ldg(SQ + (long)QUTT * NC, c);
        sq_p = ldg(SQ + PP * NC, c);
        if (!GL) sq_re = ldg(SQ + PRE * NC, c);
    }

    const double alpham = 0.5 * (dq_p / (rho * cc) - dq_un) * (rho / cc);
    const double alphap = 0.5 * (dq_p / (rho * cc) + dq_un) * (rho / cc);
    const double alpha0r = dq_rho - dq_p / csq;
    const double alpha0e = dq_re - dq_p * enth;
    const double alpha0ut = dq_ut;
    const double alpha0utt = dq_utt;

    const double e0 = un - cc, e1 = un, e2 = un + cc;

    if (do_plus) {
        // right state on the i interface, trace_plm.cpp:183-236
        double ref_fac = 0.5 * (1.0 + dtdx * amin(e0, 0.0));
        double rho_ref = rho - ref_fac * dq_rho;
        double un_ref = un - ref_fac * dq_un;
        double ut_ref = ut - ref_fac * dq_ut;
        double utt_ref = utt - ref_fac * dq_utt;
        double p_ref = p - ref_fac * dq_p;
        double rhoe_ref = rhoe - ref_fac * dq_re;

        double trace_fac0 = 0.0;
        double trace_fac1 = 0.25 * dtdx * (e0 - e1) * (1.0 - copysign(1.0, e1));
        double trace_fac2 = 0.25 * dtdx * (e0 - e2) * (1.0 - copysign(1.0, e2));

        double apright = trace_fac2 * alphap;
        double amright = trace_fac0 * alpham;

        double azrright = trace_fac1 * alpha0r;
        double azeright = trace_fac1 * alpha0e;
        double azut1rght = trace_fac1 * alpha0ut;
        double azutt1rght = trace_fac1 * alpha0utt;

        double o_rho = amax(P.small_dens, rho_ref + apright + amright + azrright);
        double o_un = un_ref + (apright - amright) * cc / rho;
        double o_ut = ut_ref + azut1rght;
        double o_utt = utt_ref + azutt1rght;
        double o_p = amax(P.small_pres, p_ref + (apright + amright) * csq);
        double o_re = rhoe_ref + (apright + amright) * enth * csq + azeright;

        o_rho = o_rho + 0.5 * dt * sq_rho;
        o_rho = amax(P.small_dens, o_rho);
        o_un = o_un + 0.5 * dt * sq_un;
        o_ut = o_ut + 0.5 * dt * sq_ut;
        o_utt = o_utt + 0.5 * dt * sq_utt;
        o_re = o_re + 0.5 * dt * sq_re;
        o_p = o_p + 0.5 * dt * sq_p;

        double spzero = un >= 0.0 ? -1.0 : un * dtdx;
        double o_X = X + 0.5 * (-1.0 - spzero) * dX;

        stg(QPd + PRHO * NC, c, o_rho);
        stg(QPd + QUN * NC, c, o_un);
        stg(QPd + QUT * NC, c, o_ut);
        stg(QPd + QUTT * NC, c, o_utt);
        stg(QPd + PP * NC, c, o_p);
        if (!GL) { stg(QPd + PRE * NC, c, o_re); stg(QPd + PX * NC, c, o_X); }
        if (lo_bc_test) {
            // Castro_ctu.cpp:293-318: the left state on the Symmetry face mirrors the right one
            stg(QMd + PRHO * NC, c, o_rho);
            stg(QMd + QUN * NC, c, -o_un);
            stg(QMd + QUT * NC, c, o_ut);
            stg(QMd + QUTT * NC, c, o_utt);
            stg(QMd + PP * NC, c, o_p);
            if (!GL) { stg(QMd + PRE * NC, c, o_re); stg(QMd + PX * NC, c, o_X); }
        }
    }

    if (do_minus) {
        // left state on the i+1 interface, trace_plm.cpp:238-300
        double ref_fac = 0.5 * (1.0 - dtdx * amax(e2, 0.0));
        double rho_ref = rho + ref_fac * dq_rho;
        double un_ref = un + ref_fac * dq_un;
        double ut_ref = ut + ref_fac * dq_ut;
        double utt_ref = utt + ref_fac * dq_utt;
        double p_ref = p + ref_fac * dq_p;
        double rhoe_ref = rhoe + ref_fac * dq_re;

        double trace_fac0 = 0.25 * dtdx * (e2 - e0) * (1.0 + copysign(1.0, e0));
        double trace_fac1 = 0.25 * dtdx * (e2 - e1) * (1.0 + copysign(1.0, e1));
        double trace_fac2 = 0.0;

        double apleft = trace_fac2 * alphap;
        double amleft = trace_fac0 * alpham;

        double azrleft = trace_fac1 * alpha0r;
        double azeleft = trace_fac1 * alpha0e;
        double azut1left = trace_fac1 * alpha0ut;
        double azutt1left = trace_fac1 * alpha0utt;

        double o_rho = amax(P.small_dens, rho_ref + apleft + amleft + azrleft);
        double o_un = un_ref + (apleft - amleft) * cc / rho;
        double o_ut = ut_ref + azut1left;
        double o_utt = utt_ref + azutt1left;
        double o_p = amax(P.small_pres, p_ref + (apleft + amleft) * csq);
        double o_re = rhoe_ref + (apleft + amleft) * enth * csq + azeleft;

        o_rho = amax(P.small_dens, o_rho + 0.5 * dt * sq_rho);
        o_un = o_un + 0.5 * dt * sq_un;
        o_ut = o_ut + 0.5 * dt * sq_ut;
        o_utt = o_utt + 0.5 * dt * sq_utt;
        o_re = o_re + 0.5 * dt * sq_re;
        o_p = o_p + 0.5 * dt * sq_p;

        double spzero = un >= 0.0 ? un * dtdx : 1.0;
        double acmpleft = 0.5 * (1.0 - spzero) * dX;
        double o_X = X + acmpleft;

        const unsigned cp = c + sd;
        stg(QMd + PRHO * NC, cp, o_rho);
        stg(QMd + QUN * NC, cp, o_un);
        stg(QMd + QUT * NC, cp, o_ut);
        stg(QMd + QUTT * NC, cp, o_utt);
        stg(QMd + PP * NC, cp, o_p);
        if (!GL) { stg(QMd + PRE * NC, cp, o_re); stg(QMd + PX * NC, cp, o_X); }
        if (hi_bc_test) {
            // Castro_ctu.cpp:320-345
            stg(QPd + PRHO * NC, cp, o_rho);
            stg(QPd + QUN * NC, cp, -o_un);
            stg(QPd + QUT * NC, cp, o_ut);
            stg(QPd + QUTT * NC, cp, o_utt);
            stg(QPd + PP * NC, cp, o_p);
            if (!GL) { stg(QPd + PRE * NC, cp, o_re); stg(QPd + PX * NC, cp, o_X); }
        }
    }
}

template <bool SRC, bool PLM, bool GL = false, bool LV = false>
__global__ void __launch_bounds__(256) k_trace(Tile t, LinBox b, const double* __restrict__ Q, DevScratch S, DevGeom g,
                                               double dt, DevParams P, LevelTab lv)
{
    unsigned vb = blockIdx.x;
    if (LV) { const LevelBox& B = level_box(lv, vb); t = B.t; b = B.bs[1]; S = B.S; Q = B.S.Q; }      // see k_src_to_prim
    int i, j, k;
    if (!box_thread_at(b, vb, threadIdx.x, i, j, k)) return;
    if (P.dtp) dt = P.dtp[6];
    const unsigned c = goff(t, i, j, k);
    const Str s = gstr(t);

    // flattening coefficient of this zone (Castro_ctu_hydro.cpp:228-266)
    double flat;
    if (P.first_order_hydro == 1) {
        flat = 0.0;
    } else if (P.use_flattening == 1) {
        const double* Pp = Q + PP * t.NC;
        double pv[7], uv[5];
        {
            const double* Uu = Q + PU * t.NC;
#pragma unroll
            for (int m = -3; m <= 3; ++m) pv[m + 3] = ldg(Pp, c + m * s.x);
#pragma unroll
            for (int m = -2; m <= 2; ++m) uv[m + 2] = ldg(Uu, c + m * s.x);
            flat = flatten_1d(pv, uv);
        }
        {
            const double* Uu = Q + PV * t.NC;
#pragma unroll
            for (int m = -3; m <= 3; ++m) pv[m + 3] = ldg(Pp, c + m * s.y);
#pragma unroll
            for (int m = -2; m <= 2; ++m) uv[m + 2] = ldg(Uu, c + m * s.y);
            flat = amin(flat, flatten_1d(pv, uv));
        }
        {
            const double* Uu = Q + PW * t.NC;
#pragma unroll
            for (int m = -3; m <= 3; ++m) pv[m + 3] = ldg(Pp, c + m * s.z);
#pragma unroll
            for (int m = -2; m <= 2; ++m) uv[m + 2] = ldg(Uu, c + m * s.z);
            flat = amin(flat, flatten_1d(pv, uv));
        }
    } else {
        flat = 1.0;
    }

    if (PLM) {
        trace_plm_dir<0, SRC, GL>(t, Q, S.SRCQ, c, s.x, i, g, flat, dt, P, i >= t.lo[0], i <= t.hi[0], S.QM[0], S.QP[0]);
        trace_plm_dir<1, SRC, GL>(t, Q, S.SRCQ, c, s.y, j, g, flat, dt, P, j >= t.lo[1], j <= t.hi[1], S.QM[1], S.QP[1]);
        trace_plm_dir<2, SRC, GL>(t, Q, S.SRCQ, c, s.z, k, g, flat, dt, P, k >= t.lo[2], k <= t.hi[2], S.QM[2], S.QP[2]);
    } else {
        const double hdt = 0.5 * dt;
        trace_dir<0, SRC, GL>(t, Q, S.SRCQ, c, s.x, flat, dt / g.dx[0], hdt, P, i >= t.lo[0], i <= t.hi[0], S.QM[0], S.QP[0]);
        trace_dir<1, SRC, GL>(t, Q, S.SRCQ, c, s.y, flat, dt / g.dx[1], hdt, P, j >= t.lo[1], j <= t.hi[1], S.QM[1], S.QP[1]);
        trace_dir<2, SRC, GL>(t, Q, S.SRCQ, c, s.z, flat, dt / g.dx[2], hdt, P, k >= t.lo[2], k <= t.hi[2], S.QM[2], S.QP[2]);
    }
}

// ---------------------------------------------------------------------------------------
// helpers shared by the Riemann stages
// ---------------------------------------------------------------------------------------
template <int D, bool NOPRE = false>
__device__ __forceinline__ void load_rstate(const double* __restrict__ E, long NC, unsigned c, double gamc,
                                            RState& q, double& X)
{
    q.rho = ldg(E + PRHO * NC, c);
    q.un = ldg(E + (PU + RDir<D>::n) * NC, c);
    q.ut = ldg(E + (PU + RDir<D>::t) * NC, c);
    q.utt = ldg(E + (PU + RDir<D>::tt) * NC, c);
    q.p = ldg(E + PP * NC, c);
    q.rhoe = NOPRE ? q.p * (1.0 / (gamc - 1.0)) : ldg(E + PRE * NC, c);       // gamma_law_edges: gamc is eos_gamma
    q.gamc = gamc;
    X = NOPRE ? 1.0 : ldg(E + PX * NC, c);
}

template <int D>
__device__ __forceinline__ void rstate_from_edge(const double q[NEDGE], double gamc, RState& r, double& X)
{
    r.rho = q[PRHO];
    r.un = q[PU + RDir<D>::n];
    r.ut = q[PU + RDir<D>::t];
    r.utt = q[PU + RDir<D>::tt];
    r.p = q[PP];
    r.rhoe = q[PRE];
    r.gamc = gamc;
    X = q[PX];
}

// wall factor of riemann_state (riemann_solvers.H:1341-1361)
template <int D>
__device__ __forceinline__ double wall_fac(const DevGeom& g, int idx)
{
    return ((idx == g.domlo[D] && g.wall_lo[D]) || (idx == g.domhi[D] + 1 && g.wall_hi[D])) ? 0.0 : 1.0;
}

// is_shock of cmpflx_plus_godunov (riemann.cpp:155-163)
__device__ __forceinline__ bool face_shock(const DevScratch& S, const DevParams& P, unsigned c, unsigned sd)
{
    if (P.hybrid_riemann != 1) return false;
    return static_cast<int>(ldg(S.SHK, c - sd) + ldg(S.SHK, c)) >= 1;
}

// Records of the transverse stages.  Two forms:
//   flux form (8 planes): the six fluxes in global component order + Godunov normal velocity and pressure;
//   state form (QI, 7 planes): the interface state (rho, un, ut, utt, p, rho e, X) the CGF solver returned -- the fluxes
//     are recomputed from it by the reader with compute_flux_q's expressions (riemann_solvers.H:14-211, as in
//     interface_flux), bit for bit: one plane less per record to write and to read (F1[x] 8 -> 7, F2 48 -> 42 planes).
//     Only where every kernel of the call is the default-solver instantiation (GEN == 0, see launch_ctu_hydro: `solv`):
//     the HLLC / HLL fluxes are not functions of one interface state.
#ifdef FLUX_FORM_ONLY            // A/B: every record in the 8-plane flux form
constexpr bool kQI = false;
#else
constexpr bool kQI = true;
#endif
constexpr int QRHO = 0, QUN = 1, QUT = 2, QUTT = 3, QPG = 4, QREG = 5, QXG = 6, NQI = 7;

template <int D>
__device__ __forceinline__ void qstate_to_rec(double rho, double un, double ut, double utt, double p, double rhoe, double Xg,
                                              double r[NF1])
{
    // interface_flux (hydro_device.h) after the Riemann solve, same order of operations
    const double frho = rho * un;
    double fmn = frho * un;
    const double fmt = frho * ut;
    const double fmtt = frho * utt;
    fmn += p;
    const double rhoetot = rhoe + 0.5 * rho * (un * un + ut * ut + utt * utt);
    r[FRHO] = frho;
    r[FMX + RDir<D>::n] = fmn;
    r[FMX + RDir<D>::t] = fmt;
    r[FMX + RDir<D>::tt] = fmtt;
    r[FE] = un * (rhoetot + p);
    r[FX] = frho * Xg;
    r[FUG] = un;
    r[FPG] = p;
}

// write a transverse-stage flux record at face offset c (global component order)
// FEI: plane of the (rho e) flux, nullptr unless transverse_reset_rhoe = 1
// NORE (first-stage records of the gamma_law_edges path): the Godunov (rho e) of a solve whose two input states have
// (rho e) = p / (gamma - 1) is the Godunov p over (gamma - 1) -- entho = 1 / (gamma - 1), estar = pstar / (gamma - 1), and the
// blend with the upwind state keeps the ratio (riemannus) -- so its plane is neither written nor read (load_f1_2)
template <int D, bool QI = false, bool NORE = false>
__device__ __forceinline__ void store_f1(double* __restrict__ F, long NC, unsigned c, const IFlux& f, double* __restrict__ FEI = nullptr)
{
    if (QI) {
        stg(F + QRHO * NC, c, f.rho_g);
        stg(F + QUN * NC, c, f.ugd);
        stg(F + QUT * NC, c, f.ut);
        stg(F + QUTT * NC, c, f.utt);
        stg(F + QPG * NC, c, f.pgd);
        if (!NORE) stg(F + QREG * NC, c, f.rhoe_g);
        if (!gamma_law_edges(0)) stg(F + QXG * NC, c, f.X_g);         // state form implies GEN == 0
        return;
    }
    if (FEI) stg(FEI, c, f.eint);
    stg(F + FRHO * NC, c, f.rho);
    stg(F + (FMX + RDir<D>::n) * NC, c, f.mn);
    stg(F + (FMX + RDir<D>::t) * NC, c, f.mt);
    stg(F + (FMX + RDir<D>::tt) * NC, c, f.mtt);
    stg(F + FE * NC, c, f.E);
    stg(F + FX * NC, c, f.X);
    stg(F + FUG * NC, c, f.ugd);
    stg(F + FPG * NC, c, f.pgd);
}

__device__ __forceinline__ void load_f1(const double* __restrict__ F, long NC, unsigned c, double r[NF1])
{
#pragma unroll
    for (int n = 0; n < NF1; ++n) r[n] = ldg(F + (long)n * NC, c);
}

__device__ __forceinline__ void load_edge(const double* __restrict__ E, long NC, unsigned c, double q[NEDGE])
{
#pragma unroll
    for (int n = 0; n < NEDGE; ++n) q[n] = ldg(E + (long)n * NC, c);
}

__host__ __device__ constexpr int f2_slot(int N, int T) { return N * 2 + ((T > N) ? T - 1 : T); }

// pair (two x-adjacent faces) forms of the record loads / stores; D: the direction the record's face is normal to
template <int D = 0, bool QI = false, bool NORE = false>
__device__ __forceinline__ void load_f1_2(const double* __restrict__ F, long NC, unsigned c, double r[2][NF1], double g1inv = 0.0)
{
    if (QI) {
        double q[2][NQI];
#pragma unroll
        for (int n = 0; n < NQI; ++n) {
            if (gamma_law_edges(0) && n == QXG) { q[0][n] = q[1][n] = 1.0; continue; }     // species elided (gamma_law_edges)
            if (NORE && n == QREG) continue;                                                // see store_f1
            const D2 v = ldg2(F + (long)n * NC, c); q[0][n] = v.a; q[1][n] = v.b;
        }
        if (NORE) { q[0][QREG] = q[0][QPG] * g1inv; q[1][QREG] = q[1][QPG] * g1inv; }
#pragma unroll
        for (int w = 0; w < 2; ++w)
            qstate_to_rec<D>(q[w][QRHO], q[w][QUN], q[w][QUT], q[w][QUTT], q[w][QPG], q[w][QREG], q[w][QXG], r[w]);
        return;
    }
#pragma unroll
    for (int n = 0; n < NF1; ++n) { const D2 v = ldg2(F + (long)n * NC, c); r[0][n] = v.a; r[1][n] = v.b; }
}

template <bool NOPRE = false>          // NOPRE (gamma_law_edges): no (rho e) plane; (rho e) = p * g1inv, g1inv = 1 / (gamma - 1)
__device__ __forceinline__ void load_edge_2(const double* __restrict__ E, long NC, unsigned c, double q[2][NEDGE], double g1inv = 0.0)
{
#pragma unroll
    for (int n = 0; n < NEDGE; ++n) {
        if (NOPRE && (n == PRE || n == PX)) continue;
#ifdef EXPERIMENT_NT_EDGE_LOADS     // an edge state is read by one thread of a kernel only
        const d2u w = __builtin_nontemporal_load(reinterpret_cast<const d2u*>(reinterpret_cast<const char*>(E + (long)n * NC) + c));
        q[0][n] = w.x; q[1][n] = w.y;
#else
        const D2 v = ldg2(E + (long)n * NC, c); q[0][n] = v.a; q[1][n] = v.b;
#endif
    }
    if (NOPRE) { q[0][PRE] = q[0][PP] * g1inv; q[1][PRE] = q[1][PP] * g1inv; q[0][PX] = q[1][PX] = 1.0; }
}

template <int D, bool QI = false, bool NORE = false>
__device__ __forceinline__ void store_f1_2(double* __restrict__ F, long NC, unsigned c, const IFlux f[2], bool m0, bool m1,
                                           double* __restrict__ FEI = nullptr)
{
    if (QI) {
        if (m0 && m1) {
            stg2(F + QRHO * NC, c, f[0].rho_g, f[1].rho_g);
            stg2(F + QUN * NC, c, f[0].ugd, f[1].ugd);
            stg2(F + QUT * NC, c, f[0].ut, f[1].ut);
            stg2(F + QUTT * NC, c, f[0].utt, f[1].utt);
            stg2(F + QPG * NC, c, f[0].pgd, f[1].pgd);
            if (!NORE) stg2(F + QREG * NC, c, f[0].rhoe_g, f[1].rhoe_g);
            if (!gamma_law_edges(0)) stg2(F + QXG * NC, c, f[0].X_g, f[1].X_g);
        } else if (m0) {
            store_f1<D, true, NORE>(F, NC, c, f[0]);
        } else if (m1) {
            store_f1<D, true, NORE>(F, NC, c + 8u, f[1]);
        }
        return;
    }
    if (FEI) {
        if (m0 && m1) stg2(FEI, c, f[0].eint, f[1].eint);
        else if (m0) stg(FEI, c, f[0].eint);
        else if (m1) stg(FEI, c + 8u, f[1].eint);
    }
    if (m0 && m1) {
        stg2(F + FRHO * NC, c, f[0].rho, f[1].rho);
        stg2(F + (FMX + RDir<D>::n) * NC, c, f[0].mn, f[1].mn);
        stg2(F + (FMX + RDir<D>::t) * NC, c, f[0].mt, f[1].mt);
        stg2(F + (FMX + RDir<D>::tt) * NC, c, f[0].mtt, f[1].mtt);
        stg2(F + FE * NC, c, f[0].E, f[1].E);
        stg2(F + FX * NC, c, f[0].X, f[1].X);
        stg2(F + FUG * NC, c, f[0].ugd, f[1].ugd);
        stg2(F + FPG * NC, c, f[0].pgd, f[1].pgd);
    } else if (m0) {
        store_f1<D>(F, NC, c, f[0]);
    } else if (m1) {
        store_f1<D>(F, NC, c + 8u, f[1]);
    }
}

// ---------------------------------------------------------------------------------------
// first Riemann solves: F^x, F^y, F^z on grow(nodal(bx,D), 1 in both transverse directions)
// (Castro_ctu_hydro.cpp:719, :796, :875)
// ---------------------------------------------------------------------------------------
// TFIX: castro.ppm_temp_fix = 2 -- the EOS fix of riemann_state on the two input states (the reference changes them
// in place; here the stored states stay as traced and every later reader applies the fix where the reference's
// order of operations has it: see trans1_body / final_body)
template <int D, bool TFIX = false, int GEN = 2, bool LV = false>
__global__ void __launch_bounds__(256) k_riemann1(Tile t, LinBox b, const double* __restrict__ Q, DevScratch S,
                                                  DevGeom g, DevParams P, LevelTab lv)
{
    unsigned vb = blockIdx.x;
    if (LV) { const LevelBox& B = level_box(lv, vb); t = B.t; b = B.bs[2]; S = B.S; Q = B.S.Q; }      // see k_src_to_prim
    int i, j, k;
    if (!box_thread_at(b, vb, threadIdx.x, i, j, k)) return;
    const bool v1 = i + 1 <= b.hi0;               // two x-adjacent faces per thread
    const unsigned c = goff(t, i, j, k);
    const unsigned sd = dstr(gstr(t), D);

    double qm[2][NEDGE], qp[2][NEDGE];
    load_edge_2<gamma_law_edges(GEN)>(S.QM[D], t.NC, c, qm, 1.0 / (P.gamma - 1.0));
    load_edge_2<gamma_law_edges(GEN)>(S.QP[D], t.NC, c, qp, 1.0 / (P.gamma - 1.0));
    if (TFIX) {
#pragma unroll
        for (int w = 0; w < 2; ++w) { temp_fix_edge(qm[w], P); temp_fix_edge(qp[w], P); }
    }
    const D2 cl = ldg2(Q + PC * t.NC, c - sd);
    const D2 cr = ldg2(Q + PC * t.NC, c);

    IFlux f[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        RState ql, qr;
        double Xl, Xr;
        rstate_from_edge<D>(qm[w], P.gamma, ql, Xl);
        rstate_from_edge<D>(qp[w], P.gamma, qr, Xr);
        const int idx = (D == 0) ? i + w : (D == 1) ? j : k;
        interface_flux<D, GEN>(ql, qr, Xl, Xr, w ? cl.b : cl.a, w ? cr.b : cr.a, wall_fac<D>(g, idx),
                          face_shock(S, P, c + 8u * w, sd), P, f[w]);
    }
    store_f1_2<D, (kQI && GEN == 0), gamma_law_edges(GEN)>(S.F1[D], t.NC, c, f, true, v1, S.F1E[D]);
}

// shared tail of the final stage for a pair of x-adjacent faces: flux in conserved order, artificial
// viscosity, species normalisation, record for consup, scaling and accumulation
//   (Castro_ctu_hydro.cpp:1192-1243, 1322-1433; apply_av advection_util.cpp:482-528;
//    normalize_species_fluxes :577-613; scale_flux :616-641)
// apply_av's coefficient for a pair of x-adjacent faces: difmag * min(0, div(u) averaged to the face)
__device__ __forceinline__ void av_div1(const DevScratch& S, unsigned c, unsigned s1, unsigned s2, const DevParams& P, double div1[2])
{
    const double* DIV = S.DIV;
    const D2 d00 = ldg2(DIV, c), d10 = ldg2(DIV, c + s1), d01 = ldg2(DIV, c + s2), d11 = ldg2(DIV, c + s1 + s2);
    div1[0] = 0.25 * (d00.a + d10.a + d01.a + d11.a);
    div1[1] = 0.25 * (d00.b + d10.b + d01.b + d11.b);
    div1[0] = P.difmag * (kAsmMinMax ? amin_hw(0.0, div1[0]) : amin(0.0, div1[0]));
    div1[1] = P.difmag * (kAsmMinMax ? amin_hw(0.0, div1[1]) : amin(0.0, div1[1]));
}

// The `assign` argument of the final kernels: bit 0 = assign (else accumulate) the fluxes; bit 1 = the old state of apply_av only
// on compressive faces; bit 2 = the operands of the evolved (rho e) only where clean_zone keeps it.  LaunchKnobs::lazy_loads:
// 0 = neither, 1 = both, 2 = the first alone, 3 = the second alone (the last two for timing them apart).
__host__ __device__ constexpr bool lazy_av_on(int assign) { return (assign & 2) != 0; }
__host__ __device__ constexpr bool lazy_eint_on(int assign) { return (assign & 4) != 0; }
static int assign_word(int flags, const LaunchKnobs& K)
{
    const int l = K.lazy_loads;
    return ((flags & 2) ? 1 : 0) | ((l == 1 || l == 2) ? 2 : 0) | ((l == 1 || l == 3) ? 4 : 0);
}

// the old state of apply_av is loaded only where a face of the pair is compressive (LaunchKnobs::lazy_loads): `contract` build,
// kernels without the flux limiters (they need uR / uL anyway).  Not in the `exact` build: a skipped F + (+-0) can differ from
// the reference in the sign of a zero.
template <bool LIM> constexpr bool lazy_av() { return kContract && !LIM; }

//   div1: av_div1 of the pair, formed by the caller (early, where lazy_av: the old-state loads depend on it)
//   lazy: LaunchKnobs::lazy_loads asks for this part (lazy_av_on)
template <int N, bool LIM, bool NOX = false>      // NOX: the species flux is the mass flux (gamma_law_edges)
__device__ __forceinline__ void final_flux_tail(const Tile& t, const DevScratch& S, const IFlux f[2], unsigned c,
                                                unsigned s1, unsigned s2, const DFab& U, unsigned cu, unsigned un_,
                                                const DFab& fluxes, const DFab& mass, const DFab& qe,
                                                int i, int j, int k, double dt, double area, double dxn, double vol,
                                                int acc_hi, bool assign, bool lazy, const double div1[2], bool v0, bool v1,
                                                const DevParams& P, double R[2][NFIN])
{
    double F[2][NUM_STATE];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        F[w][URHO] = f[w].rho;
        F[w][UMX + RDir<N>::n] = f[w].mn;
        F[w][UMX + RDir<N>::t] = f[w].mt;
        F[w][UMX + RDir<N>::tt] = f[w].mtt;
        F[w][UEDEN] = f[w].E;
        F[w][UEINT] = f[w].eint;
        F[w][UTEMP] = 0.0;                       // Castro_ctu_hydro.cpp:1201
        F[w][UFS] = f[w].X;
    }

    {
        double uR[2][NUM_STATE], uL[2][NUM_STATE];            // kept only by the flux limiters
        // Where neither face is compressive div1 is zero and the term below is +-0: the six planes of U at the zone and its low
        // neighbour are not loaded (a wave without a compressive face jumps over the block).  An Inf or NaN in U on a skipped face
        // does not go unseen: the reference's term would be NaN there, and here the same zone still enters the update through u0
        // and gave the edge states of the face, so the NaN reaches S_new and nan_guard all the same.  A NaN in div(u) is dropped by
        // the hardware minimum (amin_hw(0, NaN) = 0): div1 is 0 and the block is skipped, where the term was 0 * dU before -- no
        // result changes; such a div(u) comes from NaN velocities in Q, which reach the fluxes through the edge states.
        const bool av = !lazy_av<LIM>() || !lazy || div1[0] != 0.0 || div1[1] != 0.0;
        if (av) {
#pragma unroll
        for (int m = 0; m < NUM_STATE; ++m) {
            if (m == UTEMP) { if (LIM) { uR[0][m] = uR[1][m] = uL[0][m] = uL[1][m] = 0.0; } continue; }
            const D2 uc = ldg2(U.p + m * U.sn, cu), ul = ldg2(U.p + m * U.sn, cu - un_);
            double d1 = div1[0] * (uc.a - ul.a);
            F[0][m] += dxn * d1;
            d1 = div1[1] * (uc.b - ul.b);
            F[1][m] += dxn * d1;
            if (LIM) { uR[0][m] = uc.a; uR[1][m] = uc.b; uL[0][m] = ul.a; uL[1][m] = ul.b; }
        }
        }
        if (LIM) {
            // limit_fluxes_on_small_dens / _large_vel (Castro_ctu_hydro.cpp:1219-1239), between apply_av and the
            // species normalisation; normal velocity and pressure of the zones either side of the face
            const unsigned sn = dstr(gstr(t), N);
            const D2 vr = ldg2(S.Q + (long)(PU + N) * t.NC, c), vl = ldg2(S.Q + (long)(PU + N) * t.NC, c - sn);
            const D2 pr = ldg2(S.Q + (long)PP * t.NC, c), pl = ldg2(S.Q + (long)PP * t.NC, c - sn);
            const double dtdx = dt / dxn;
            if (P.limit_small_dens == 1) {
                limit_flux_small_dens<N>(uL[0], uR[0], vl.a, pl.a, vr.a, pr.a, dt, dtdx, area, vol, P, F[0]);
                limit_flux_small_dens<N>(uL[1], uR[1], vl.b, pl.b, vr.b, pr.b, dt, dtdx, area, vol, P, F[1]);
            }
            if (P.limit_large_vel == 1) {
                limit_flux_large_vel<N>(uL[0], uR[0], vl.a, pl.a, vr.a, pr.a, dt, dtdx, area, vol, P, F[0]);
                limit_flux_large_vel<N>(uL[1], uR[1], vl.b, pl.b, vr.b, pr.b, dt, dtdx, area, vol, P, F[1]);
            }
        }
    }

#pragma unroll
    for (int w = 0; w < 2; ++w) {
        if (NOX) {
            F[w][UFS] = F[w][URHO];               // what normalize_species_fluxes makes of it for one species
        } else {
        double sum = 0.0;
        sum += F[w][UFS];
        double fac = 1.0;
        if (fabs(sum) > 2.220446049250313e-16 * fabs(F[w][URHO])) fac = F[w][URHO] / sum;
        F[w][UFS] = F[w][UFS] * fac;
        }

        // record for consup (stored by the caller, two faces per store)
        R[w][GRHO] = F[w][URHO]; R[w][GMX] = F[w][UMX]; R[w][GMY] = F[w][UMY]; R[w][GMZ] = F[w][UMZ];
        R[w][GE] = F[w][UEDEN]; R[w][GEI] = F[w][UEINT]; R[w][GX] = F[w][UFS]; R[w][GUG] = f[w].ugd; R[w][GPG] = f[w].pgd;
    }

    const int idx0 = (N == 0) ? i : (N == 1) ? j : k;
    const int idx1 = (N == 0) ? i + 1 : idx0;
    const bool m0 = v0 && idx0 <= acc_hi, m1 = v1 && idx1 <= acc_hi;
    if (m0 && m1) {
        if (fluxes.p) {
            const unsigned cf = foff(fluxes, i, j, k);
#pragma unroll
            for (int m = 0; m < NUM_STATE; ++m) {
                double* dst = fluxes.p + m * fluxes.sn;
                if (assign) {
                    // fluxes[d] was going to be zeroed by the caller (Castro_advance.cpp:391-394): 0 + x
                    stg2(dst, cf, 0.0 + dt * F[0][m] * area, 0.0 + dt * F[1][m] * area);
                } else {
                    if (m == UTEMP) continue;       // += dt*0*area leaves the register unchanged
                    const D2 old = ldg2(dst, cf);
                    stg2(dst, cf, old.a + dt * F[0][m] * area, old.b + dt * F[1][m] * area);
                }
            }
        }
        if (mass.p) stg2(mass.p, foff(mass, i, j, k), dt * F[0][URHO] * area, dt * F[1][URHO] * area);
        if (qe.p) {
            const unsigned cq = foff(qe, i, j, k);
            stg2(qe.p + (GDU + RDir<N>::n) * qe.sn, cq, f[0].ugd, f[1].ugd);
            stg2(qe.p + (GDU + RDir<N>::t) * qe.sn, cq, f[0].ut, f[1].ut);
            stg2(qe.p + (GDU + RDir<N>::tt) * qe.sn, cq, f[0].utt, f[1].utt);
            stg2(qe.p + GDPRES * qe.sn, cq, f[0].pgd, f[1].pgd);
        }
    } else {
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            if (!(w ? m1 : m0)) continue;
            if (fluxes.p) {
                const unsigned cf = foff(fluxes, i + w, j, k);
#pragma unroll
                for (int m = 0; m < NUM_STATE; ++m) {
                    double* dst = fluxes.p + m * fluxes.sn;
                    if (assign) {
                        stg(dst, cf, 0.0 + dt * F[w][m] * area);
                    } else {
                        if (m == UTEMP) continue;
                        stg(dst, cf, ldg(dst, cf) + dt * F[w][m] * area);
                    }
                }
            }
            if (mass.p) stg(mass.p, foff(mass, i + w, j, k), dt * F[w][URHO] * area);
            if (qe.p) {
                const unsigned cq = foff(qe, i + w, j, k);
                stg(qe.p + (GDU + RDir<N>::n) * qe.sn, cq, f[w].ugd);
                stg(qe.p + (GDU + RDir<N>::t) * qe.sn, cq, f[w].ut);
                stg(qe.p + (GDU + RDir<N>::tt) * qe.sn, cq, f[w].utt);
                stg(qe.p + GDPRES * qe.sn, cq, f[w].pgd);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// transverse stage 1 for normal direction N: both trans_single corrections of the N edge
// states and the Riemann solves on the corrected states.
//   F2 slot (N|T): flux in direction N from states corrected with the T-direction flux.
// (Castro_ctu_hydro.cpp:724-945 for the corrections, :949-1135 for the six solves)
// ---------------------------------------------------------------------------------------
#ifndef TRACE_SPLIT_WAVES
#define TRACE_SPLIT_WAVES 2
#endif
// device-resident time step (DevParams::dtp): cdtdx = dt/dx/3 as launch_ctu_hydro computes it on the host
#define DT_THIRDS_FROM_DEVICE()                                                                          \
    if (P.dtp) { const double dt_ = P.dtp[6]; cdtdx = dt_ / g.dx[0] / 3.0; cdtdy = dt_ / g.dx[1] / 3.0; cdtdz = dt_ / g.dx[2] / 3.0; }
template <bool XRIEM, int DMASK = 7, int GEN = 2, bool LV = false>
#ifndef TRACE_PAIR_WAVES        // A/B (round 6, profiles/r06f_*): 3 = the pair kernel held to 168 registers for a third wave per SIMD
#define TRACE_PAIR_WAVES 2
#endif
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((DMASK == 1 || DMASK == 2 || DMASK == 4) ? TRACE_SPLIT_WAVES : TRACE_PAIR_WAVES)))
k_trace_pair(Tile t, LinBox b, const double* __restrict__ Q, DevScratch S, DevGeom g,
                                                    double dt, DevParams P, SkipBox skip, LevelTab lv, int with_divu)
{
    constexpr bool GL = gamma_law_edges(GEN) && DMASK == 7;
    if (P.dtp) dt = P.dtp[6];
    unsigned vb = blockIdx.x;
    if (LV) { const LevelBox& B = level_box(lv, vb); t = B.t; b = B.b[LB_TRACE]; S = B.S; Q = B.S.Q; }
    int i, j, k;
    bool valid = box_thread_at(b, vb, threadIdx.x, i, j, k);           // no early exit when XRIEM: the block synchronises below
    if (!valid) { i = b.lo[0]; j = b.lo[1]; k = b.lo[2]; }
    bool v1 = valid && i + 1 <= b.hi0;
    if (!XRIEM) {
        // staged execution: zones of the skip box belong to the other launch
        const bool s0 = in_skip(skip, i, j, k), s1 = in_skip(skip, i + 1, j, k);
        if ((!valid || s0) && (!v1 || s1)) return;
        if (s1) v1 = false;
        if (s0) valid = false;
    }
    const unsigned c = goff(t, i, j, k);
    const Str s = gstr(t);
    const long NC = t.NC;

    // Castro::divu (advection_util.cpp:458-475) for the low nodes of the two zones, in front of the tracing: the launch covers the
    // box k_divu_pair would cover, its registers are free again before the stencils below are requested, and the velocities
    // it reads are planes this kernel streams anyway (round 6: a launch of 0.18 ms at 256^3 folded in)
    if (with_divu && valid) divu_pair_body(t, Q, S.DIV, c, v1, 1.0 / g.dx[0], 1.0 / g.dx[1], 1.0 / g.dx[2]);

    // flattening coefficients of the two zones (Castro_ctu_hydro.cpp:228-266)
    double flat[2];
#ifdef TRACE_DIAG_NOFLAT      // timing diagnostic (wrong results): no flattening stencils
    if (P.first_order_hydro != 2) {
        flat[0] = flat[1] = 1.0;
    } else
#endif
    if (P.first_order_hydro == 1) {
        flat[0] = flat[1] = 0.0;
    } else if (P.use_flattening == 1) {
        // all three directions' stencils are requested before the first coefficient is evaluated
        const double* Pp = Q + PP * NC;
        double pxA[7], pxB[7], uxA[5], uxB[5], pyA[7], pyB[7], uyA[5], uyB[5], pzA[7], pzB[7], uzA[5], uzB[5];
        {
            const D2 p0 = ldg2(Pp, c - 24u), p1 = ldg2(Pp, c - 8u), p2 = ldg2(Pp, c + 8u), p3 = ldg2(Pp, c + 24u);
            pxA[0] = p0.a; pxA[1] = p0.b; pxA[2] = p1.a; pxA[3] = p1.b; pxA[4] = p2.a; pxA[5] = p2.b; pxA[6] = p3.a;
            pxB[0] = p0.b; pxB[1] = p1.a; pxB[2] = p1.b; pxB[3] = p2.a; pxB[4] = p2.b; pxB[5] = p3.a; pxB[6] = p3.b;
            load_stencil_2<0>(Q + PU * NC, c, s.x, uxA, uxB);
        }
#pragma unroll
        for (int m = -3; m <= 3; ++m) { const D2 v = ldg2(Pp, c + m * s.y); pyA[m + 3] = v.a; pyB[m + 3] = v.b; }
        load_stencil_2<1>(Q + PV * NC, c, s.y, uyA, uyB);
#pragma unroll
        for (int m = -3; m <= 3; ++m) { const D2 v = ldg2(Pp, c + m * s.z); pzA[m + 3] = v.a; pzB[m + 3] = v.b; }
        load_stencil_2<2>(Q + PW * NC, c, s.z, uzA, uzB);
        flat[0] = flatten_1d(pxA, uxA);
        flat[1] = flatten_1d(pxB, uxB);
        flat[0] = amin_c(flat[0], flatten_1d(pyA, uyA));
        flat[1] = amin_c(flat[1], flatten_1d(pyB, uyB));
        flat[0] = amin_c(flat[0], flatten_1d(pzA, uzA));
        flat[1] = amin_c(flat[1], flatten_1d(pzB, uzB));
    } else {
        flat[0] = flat[1] = 1.0;
    }

    bool dp[2], dm[2];
    double qp[2][NEDGE], qm[2][NEDGE];
    dp[0] = valid && i >= t.lo[0]; dp[1] = v1 && i + 1 >= t.lo[0];
    dm[0] = valid && i <= t.hi[0]; dm[1] = v1 && i + 1 <= t.hi[0];
    double sa[2][5], sb[2][5];
    if (DMASK & 1) {
        load_stencil_2<0>(Q + (long)PU * NC, c, s.x, sa[0], sa[1]);
        load_stencil_2<0>(Q + (long)PRHO * NC, c, s.x, sb[0], sb[1]);
        trace_pair_dir<0, (DMASK & 2) ? 1 : -1, GL>(t, Q, c, s.x, s.y, flat, dt / g.dx[0], P, dp, dm, S.QM[0], S.QP[0], qp, qm, sa[0], sa[1], sb[0], sb[1]);
    }

    if (XRIEM && (DMASK & 1))
    // ---- first Riemann solve in x (Castro_ctu_hydro.cpp:719) on the two faces of this thread:
    //      face i+1 lies between its two zones; face i needs the minus state of the zone to the left, which
    //      the neighbouring lane (or, across a wavefront boundary, LDS) hands over.  The first thread of a
    //      workgroup has no left neighbour here: k_riemann1_blockstart does those faces from QM/QP.
    {
        double qmL[NEDGE];
        __shared__ double xch[4][NEDGE];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int n = 0; n < NEDGE; ++n) qmL[n] = __shfl_up(qm[1][n], 1, 64);
        if (lane == 63) {
#pragma unroll
            for (int n = 0; n < NEDGE; ++n) xch[wave][n] = qm[1][n];
        }
        __syncthreads();
        if (lane == 0 && wave > 0) {
#pragma unroll
            for (int n = 0; n < NEDGE; ++n) qmL[n] = xch[wave - 1][n];
        }
        // face i (plus state: zone i): the left neighbour must be a thread of this row and of this workgroup
        const bool mA = valid && i >= t.lo[0] && i > b.lo[0] && threadIdx.x > 0;
        const bool mB = v1;                                            // face i+1 (needed: i+1 >= lo always)
        if (mA || mB) {
            const double* Cp = Q + PC * NC;
            const double cm1 = ldg(Cp, c - 8u);
            const D2 cc01 = ldg2(Cp, c);
            IFlux f[2];
            RState ql, qr;
            double Xl, Xr;
            rstate_from_edge<0>(qmL, P.gamma, ql, Xl);
            rstate_from_edge<0>(qp[0], P.gamma, qr, Xr);
            interface_flux<0, GEN>(ql, qr, Xl, Xr, cm1, cc01.a, wall_fac<0>(g, i), face_shock(S, P, c, 8u), P, f[0]);
            rstate_from_edge<0>(qm[0], P.gamma, ql, Xl);
            rstate_from_edge<0>(qp[1], P.gamma, qr, Xr);
            interface_flux<0, GEN>(ql, qr, Xl, Xr, cc01.a, cc01.b, wall_fac<0>(g, i + 1), face_shock(S, P, c + 8u, 8u), P, f[1]);
            store_f1_2<0, (kQI && GEN == 0), gamma_law_edges(GEN)>(S.F1[0], NC, c, f, mA, mB, S.F1E[0]);
        }
    }

    if (DMASK & 2) {
        if (!(DMASK & 1)) {
            load_stencil_2<1>(Q + (long)PV * NC, c, s.y, sb[0], sb[1]);
            load_stencil_2<1>(Q + (long)PRHO * NC, c, s.y, sa[0], sa[1]);
        }
        const bool a = j >= t.lo[1], z = j <= t.hi[1]; dp[0] = valid && a; dp[1] = v1 && a; dm[0] = valid && z; dm[1] = v1 && z;
        trace_pair_dir<1, (DMASK & 4) ? 2 : -1, GL>(t, Q, c, s.y, s.z, flat, dt / g.dx[1], P, dp, dm, S.QM[1], S.QP[1], qp, qm, sb[0], sb[1], sa[0], sa[1]);
    }
    if (DMASK & 4) {
        if (!(DMASK & 2)) {
            load_stencil_2<2>(Q + (long)PW * NC, c, s.z, sa[0], sa[1]);
            load_stencil_2<2>(Q + (long)PRHO * NC, c, s.z, sb[0], sb[1]);
        }
        const bool a = k >= t.lo[2], z = k <= t.hi[2]; dp[0] = valid && a; dp[1] = v1 && a; dm[0] = valid && z; dm[1] = v1 && z;
        trace_pair_dir<2, -1, GL>(t, Q, c, s.z, 0u, flat, dt / g.dx[2], P, dp, dm, S.QM[2], S.QP[2], qp, qm, sa[0], sa[1], sb[0], sb[1]);
#ifdef TRACE_DIAG_STORES_AT_END       // ... but as twenty more stores (of the z values) behind the z stores: same bytes, same instructions, all at the end
        if (GL) {
            store_edge_2<true>(S.QP[0], NC, c, qp, dp[0], dp[1]);
            store_edge_2<true>(S.QM[0], NC, c + s.x, qm, dm[0], dm[1]);
            store_edge_2<true>(S.QP[1], NC, c, qp, dp[0], dp[1]);
            store_edge_2<true>(S.QM[1], NC, c + s.y, qm, dm[0], dm[1]);
        }
#endif
    }
}

// the x-faces k_trace_pair leaves out: face i of the first thread of every workgroup of that launch
template <int GEN = 2, bool LV = false>
__global__ void __launch_bounds__(256) k_riemann1_blockstart(Tile t, LinBox b, const double* __restrict__ Q, DevScratch S,
                                                             DevGeom g, DevParams P, LevelTab lv)
{
    unsigned vb = blockIdx.x;
    if (LV) { const LevelBox& B = level_box(lv, vb); t = B.t; b = B.b[LB_TRACE]; S = B.S; Q = B.S.Q; }
    const unsigned blk = vb * blockDim.x + threadIdx.x;      // workgroup index of the k_trace_pair launch
    if (blk >= b.nb) return;
    int i, j, k;
    if (!box_thread_at(b, blk, 0u, i, j, k)) return;
    if (i < t.lo[0] || i == b.lo[0]) return;      // row starts are the caller's business (launch-box faces)
    const unsigned c = goff(t, i, j, k);
    RState ql, qr;
    double Xl, Xr;
    load_rstate<0, gamma_law_edges(GEN)>(S.QM[0], t.NC, c, P.gamma, ql, Xl);
    load_rstate<0, gamma_law_edges(GEN)>(S.QP[0], t.NC, c, P.gamma, qr, Xr);
    const double cl = ldg(Q + PC * t.NC, c - 8u);
    const double cr = ldg(Q + PC * t.NC, c);
    IFlux f;
    interface_flux<0, GEN>(ql, qr, Xl, Xr, cl, cr, wall_fac<0>(g, i), face_shock(S, P, c, 8u), P, f);
    store_f1<0, (kQI && GEN == 0), gamma_law_edges(GEN)>(S.F1[0], t.NC, c, f, S.F1E[0]);
}



template <int N, int T, bool RE, int GEN = 2>
__device__ __forceinline__ void trans1_pair(const Tile& t, const DevScratch& S, unsigned c, unsigned sn, unsigned st,
                                            const double qm[2][NEDGE], const double qp[2][NEDGE],
                                            const D2& cl, const D2& cr, const double bnd_fac[2], double cdtdx,
                                            bool m0, bool m1, const DevParams& P)
{
    double fr[2][NF1], fl[2][NF1], qmo[2][NEDGE], qpo[2][NEDGE];

    // minus states live in zones c - sn; their T-faces are (c - sn) and (c - sn + st)
#ifdef DIAG_F1_REUSE      // timing diagnostic (wrong results): one record load per (N,T) instead of four
    load_f1_2<T, (kQI && GEN == 0), gamma_law_edges(GEN)>(S.F1[T], t.NC, c, fl, 1.0 / (P.gamma - 1.0));
#pragma unroll
    for (int w = 0; w < 2; ++w)
#pragma unroll
        for (int n = 0; n < NF1; ++n) fr[w][n] = fl[w][n] * 1.01;
#else
#ifdef DIAG_T1_NOLOAD     // timing diagnostic (wrong results): inputs made up from the index instead of loaded
#pragma unroll
    for (int w = 0; w < 2; ++w)
#pragma unroll
        for (int n = 0; n < NF1; ++n) { fr[w][n] = 1e-3 * (double)((c + n + w) & 255u); fl[w][n] = 1e-3 * (double)((c + st + n) & 255u); }
#else
    load_f1_2<T, (kQI && GEN == 0), gamma_law_edges(GEN)>(S.F1[T], t.NC, c - sn + st, fr, 1.0 / (P.gamma - 1.0));
    load_f1_2<T, (kQI && GEN == 0), gamma_law_edges(GEN)>(S.F1[T], t.NC, c - sn, fl, 1.0 / (P.gamma - 1.0));
#endif
#endif
    if (RE && P.reset_rhoe == 1) {                 // transverse_reset_rhoe = 1: the (rho e) flux differences as well
        const D2 er = ldg2(S.F1E[T], c - sn + st), el = ldg2(S.F1E[T], c - sn);
        trans_single<T>(qm[0], fr[0], fl[0], P.gamma, cdtdx, P, qmo[0], er.a, el.a);
        trans_single<T>(qm[1], fr[1], fl[1], P.gamma, cdtdx, P, qmo[1], er.b, el.b);
    } else {
#pragma unroll
        for (int w = 0; w < 2; ++w) trans_single<T>(qm[w], fr[w], fl[w], P.gamma, cdtdx, P, qmo[w]);
    }

    // plus states live in zones c
#if !defined(DIAG_F1_REUSE) && !defined(DIAG_T1_NOLOAD)
    load_f1_2<T, (kQI && GEN == 0), gamma_law_edges(GEN)>(S.F1[T], t.NC, c + st, fr, 1.0 / (P.gamma - 1.0));
    load_f1_2<T, (kQI && GEN == 0), gamma_law_edges(GEN)>(S.F1[T], t.NC, c, fl, 1.0 / (P.gamma - 1.0));
#endif
    if (RE && P.reset_rhoe == 1) {
        const D2 er = ldg2(S.F1E[T], c + st), el = ldg2(S.F1E[T], c);
        trans_single<T>(qp[0], fr[0], fl[0], P.gamma, cdtdx, P, qpo[0], er.a, el.a);
        trans_single<T>(qp[1], fr[1], fl[1], P.gamma, cdtdx, P, qpo[1], er.b, el.b);
    } else {
#pragma unroll
        for (int w = 0; w < 2; ++w) trans_single<T>(qp[w], fr[w], fl[w], P.gamma, cdtdx, P, qpo[w]);
    }

    if (RE && P.ppm_temp_fix == 2 && P.riemann_solver != 2) {
#pragma unroll
        for (int w = 0; w < 2; ++w) { temp_fix_edge(qmo[w], P); temp_fix_edge(qpo[w], P); }
    }
    IFlux f[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
#ifdef DIAG_T1_NOSOLVE    // timing diagnostic (wrong results): the Riemann solve replaced by sums of its inputs
        f[w].rho = qmo[w][PRHO] + qpo[w][PRHO]; f[w].mn = qmo[w][PU] + qpo[w][PU]; f[w].mt = qmo[w][PV] + qpo[w][PV];
        f[w].mtt = qmo[w][PW] + qpo[w][PW]; f[w].E = qmo[w][PP] + qpo[w][PP]; f[w].eint = qmo[w][PRE] + qpo[w][PRE];
        f[w].X = qmo[w][PX] + qpo[w][PX]; f[w].ugd = (w ? cl.b : cl.a) + bnd_fac[w]; f[w].pgd = (w ? cr.b : cr.a);
        f[w].ut = 0.0; f[w].utt = 0.0;
#else
        RState ql, qr;
        double Xl, Xr;
        rstate_from_edge<N>(qmo[w], P.gamma, ql, Xl);
        rstate_from_edge<N>(qpo[w], P.gamma, qr, Xr);
        interface_flux<N, GEN>(ql, qr, Xl, Xr, w ? cl.b : cl.a, w ? cr.b : cr.a, bnd_fac[w],
                          face_shock(S, P, c + 8u * w, sn), P, f[w]);
#ifdef DIAG_T1_EXTRA_SOLVES   // timing diagnostic (wrong results): DIAG_T1_EXTRA_SOLVES more Riemann solves per face and (N,T), on
                              // perturbed states so that they are not merged: what "recompute instead of store" costs this kernel
#pragma unroll
        for (int x = 0; x < DIAG_T1_EXTRA_SOLVES; ++x) {
            IFlux fx;
            ql.rho = ql.rho * 1.0000001 + 1e-12 * f[w].rho; qr.p = qr.p * 0.9999999 + 1e-12 * f[w].pgd;
            interface_flux<N, GEN>(ql, qr, Xl, Xr, w ? cl.b : cl.a, w ? cr.b : cr.a, bnd_fac[w],
                              face_shock(S, P, c + 8u * w, sn), P, fx);
            f[w].rho += 1e-30 * fx.rho; f[w].mn += 1e-30 * fx.mn; f[w].E += 1e-30 * fx.E; f[w].ugd += 1e-30 * fx.ugd; f[w].pgd += 1e-30 * fx.pgd;
        }
#endif
#endif
    }
#ifdef DIAG_T1_NOSTORE    // timing diagnostic: the stores behind a condition that never holds
    if (f[0].rho == 1.2345e300)
#endif
    store_f1_2<N, (kQI && GEN == 0)>(S.F2[f2_slot(N, T)], t.NC, c, f, m0, m1, RE ? S.F2E[f2_slot(N, T)] : nullptr);
}

// one normal direction of the transverse stage for the faces (ijk) and (ijk + x) -- `v1`: the second face exists
template <int N, bool RE, int GEN = 2>
__device__ __forceinline__ void trans1_body(const Tile& t, const int ijk[3], bool v1, unsigned c,
                                            const double* __restrict__ Q, const DevScratch& S, const DevGeom& g,
                                            double cdtdx_t1, double cdtdx_t2, const DevParams& P)
{
    constexpr int T1 = (N == 0) ? 1 : 0;
    constexpr int T2 = (N == 2) ? 1 : 2;
    const Str s = gstr(t);
    const unsigned sn = dstr(s, N);

    // the (N|T1) states exist where the T1 index is inside bx (T2 index may be in the 1-ring); the N-face
    // itself must belong to grow(nodal(bx, N), 1 in T1 and T2)
    bool in_t1[2], in_t2[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const int i1 = ijk[T1] + (T1 == 0 ? w : 0), i2 = ijk[T2] + (T2 == 0 ? w : 0);
        const int in = ijk[N] + (N == 0 ? w : 0);
        const bool v = ((w == 0) || v1) && in >= t.lo[N];
        in_t1[w] = v && i1 >= t.lo[T1] && i1 <= t.hi[T1];
        in_t2[w] = v && i2 >= t.lo[T2] && i2 <= t.hi[T2];
    }
    const bool any1 = in_t1[0] || in_t1[1], any2 = in_t2[0] || in_t2[1];
    if (!any1 && !any2) return;

    double qm[2][NEDGE], qp[2][NEDGE];
#ifdef DIAG_T1_NOLOAD
    D2 cl, cr;
    cl.a = cl.b = cr.a = cr.b = 1.3;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const double e = 1e-6 * (double)((c + w) & 255u);
        qm[w][PRHO] = 1.0 + e; qm[w][PU] = 0.1; qm[w][PV] = 0.2 + e; qm[w][PW] = 0.3; qm[w][PP] = 1.0 + e; qm[w][PRE] = 2.5; qm[w][PX] = 1.0;
        qp[w][PRHO] = 1.1 + e; qp[w][PU] = 0.2; qp[w][PV] = 0.1 + e; qp[w][PW] = 0.2; qp[w][PP] = 1.1 + e; qp[w][PRE] = 2.75; qp[w][PX] = 1.0;
    }
#else
    load_edge_2<gamma_law_edges(GEN)>(S.QM[N], t.NC, c, qm, 1.0 / (P.gamma - 1.0));
    load_edge_2<gamma_law_edges(GEN)>(S.QP[N], t.NC, c, qp, 1.0 / (P.gamma - 1.0));
    const D2 cl = ldg2(Q + PC * t.NC, c - sn);
    const D2 cr = ldg2(Q + PC * t.NC, c);
#endif
    double bnd_fac[2];
    bnd_fac[0] = wall_fac<N>(g, ijk[N]);
    bnd_fac[1] = wall_fac<N>(g, ijk[N] + (N == 0 ? 1 : 0));

    if (RE && P.ppm_temp_fix == 2 && P.riemann_solver != 2) {
        // The reference's first solves change their input states in place, in the order x, y, z, each followed by the
        // transverse corrections that use its flux (Castro_ctu_hydro.cpp:719-945): the N states corrected with the T
        // flux have been through their own first solve by then iff N comes before T.
        double qmf[2][NEDGE], qpf[2][NEDGE];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
            for (int n = 0; n < NEDGE; ++n) { qmf[w][n] = qm[w][n]; qpf[w][n] = qp[w][n]; }
            temp_fix_edge(qmf[w], P); temp_fix_edge(qpf[w], P);
        }
        if (any1) trans1_pair<N, T1, RE, GEN>(t, S, c, sn, dstr(s, T1), (N < T1) ? qmf : qm, (N < T1) ? qpf : qp, cl, cr, bnd_fac,
                                         cdtdx_t1, in_t1[0], in_t1[1], P);
        if (any2) trans1_pair<N, T2, RE, GEN>(t, S, c, sn, dstr(s, T2), (N < T2) ? qmf : qm, (N < T2) ? qpf : qp, cl, cr, bnd_fac,
                                         cdtdx_t2, in_t2[0], in_t2[1], P);
        return;
    }
    if (any1) trans1_pair<N, T1, RE, GEN>(t, S, c, sn, dstr(s, T1), qm, qp, cl, cr, bnd_fac, cdtdx_t1, in_t1[0], in_t1[1], P);
    if (any2) trans1_pair<N, T2, RE, GEN>(t, S, c, sn, dstr(s, T2), qm, qp, cl, cr, bnd_fac, cdtdx_t2, in_t2[0], in_t2[1], P);
}

// ---------------------------------------------------------------------------------------
// k_trans1 with the first y and z Riemann solves folded in (default solver, no transverse_reset_rhoe / ppm_temp_fix):
// F1[y] and F1[z] are never written.  The transverse stage reads QM/QP[y], QM/QP[z] anyway; a thread solves the four
// y-faces and the four z-faces of its two zones itself (records A), takes those of the zone to its left from the
// neighbouring lane (one wave shuffle per component; consecutive waves overlap by one slot, so lane 0 of a wave only
// gives), and re-solves those of the zones below in the other transverse direction (records B).  8 first solves per
// zone instead of 2 -- k_trans1's arithmetic hides under its memory traffic (profiles/r03b_ab_trans1_extra_solves.txt:
// +6 solves per zone cost 0.5 ms) -- against two k_riemann1 launches (1.36 ms, 46 plane passes) and 16 planes less
// to read here.  The arithmetic per face is that of k_riemann1: bit-identical F2.
// ---------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void flux_to_rec(const IFlux& f, double r[NF1])
{
    r[FRHO] = f.rho;
    r[FMX + RDir<D>::n] = f.mn;
    r[FMX + RDir<D>::t] = f.mt;
    r[FMX + RDir<D>::tt] = f.mtt;
    r[FE] = f.E;
    r[FX] = f.X;
    r[FUG] = f.ugd;
    r[FPG] = f.pgd;
}

// first Riemann solve on the D-faces of the two zones of a pair from their edge states (cmpflx_plus_godunov, riemann.cpp:15-206)
template <int D, int GEN>
__device__ __forceinline__ void f1_solve_2(const double qm[2][NEDGE], const double qp[2][NEDGE], const D2& cl, const D2& cr,
                                           double bnd, const DevParams& P, double r[2][NF1])
{
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        RState ql, qr;
        double Xl, Xr;
        rstate_from_edge<D>(qm[w], P.gamma, ql, Xl);
        rstate_from_edge<D>(qp[w], P.gamma, qr, Xr);
        IFlux f;
        interface_flux<D, GEN>(ql, qr, Xl, Xr, w ? cl.b : cl.a, w ? cr.b : cr.a, bnd, false, P, f);
        flux_to_rec<D>(f, r[w]);
#ifndef FOLD_NO_SCHED_BARRIER
        __builtin_amdgcn_sched_barrier(0);        // one zone's solve at a time: the two interleaved cost ~50 more registers
#endif
    }
}

// ... with the edge states and sound speeds of the faces at offset cf loaded here; idx: index of those faces along D
template <int D, int GEN>
__device__ __forceinline__ void f1_at_2(const Tile& t, const double* __restrict__ Q, const DevScratch& S, const DevGeom& g,
                                        const DevParams& P, unsigned cf, int idx, double r[2][NF1])
{
    double qm[2][NEDGE], qp[2][NEDGE];
    load_edge_2<gamma_law_edges(GEN)>(S.QM[D], t.NC, cf, qm, 1.0 / (P.gamma - 1.0));
    load_edge_2<gamma_law_edges(GEN)>(S.QP[D], t.NC, cf, qp, 1.0 / (P.gamma - 1.0));
    const unsigned sd = dstr(gstr(t), D);
    const D2 cl = ldg2(Q + PC * t.NC, cf - sd), cr = ldg2(Q + PC * t.NC, cf);
    f1_solve_2<D, GEN>(qm, qp, cl, cr, wall_fac<D>(g, idx), P, r);
}

// ... with the sound speeds either side handed in (the caller has them already)
template <int D, int GEN>
__device__ __forceinline__ void f1_at_2c(const Tile& t, const DevScratch& S, const DevGeom& g, const DevParams& P, unsigned cf, int idx,
                                         const D2& cl, const D2& cr, double r[2][NF1])
{
    double qm[2][NEDGE], qp[2][NEDGE];
    load_edge_2<gamma_law_edges(GEN)>(S.QM[D], t.NC, cf, qm, 1.0 / (P.gamma - 1.0));
    load_edge_2<gamma_law_edges(GEN)>(S.QP[D], t.NC, cf, qp, 1.0 / (P.gamma - 1.0));
    f1_solve_2<D, GEN>(qm, qp, cl, cr, wall_fac<D>(g, idx), P, r);
}

// second-stage Riemann solve of trans1_pair on already corrected states
template <int N, int T, int GEN>
__device__ __forceinline__ void trans1_solve_store(const Tile& t, const DevScratch& S, unsigned c,
                                                   const double qmo[2][NEDGE], const double qpo[2][NEDGE],
                                                   const D2& cl, const D2& cr, const double bnd_fac[2],
                                                   bool m0, bool m1, const DevParams& P)
{
    IFlux f[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        RState ql, qr;
        double Xl, Xr;
        rstate_from_edge<N>(qmo[w], P.gamma, ql, Xl);
        rstate_from_edge<N>(qpo[w], P.gamma, qr, Xr);
        interface_flux<N, GEN>(ql, qr, Xl, Xr, w ? cl.b : cl.a, w ? cr.b : cr.a, bnd_fac[w], false, P, f[w]);
    }
#ifdef DIAG_T1_NOSTORE    // timing diagnostic: the stores behind a condition that never holds
    if (f[0].rho == 1.2345e300)
#endif
    store_f1_2<N, (kQI && GEN == 0)>(S.F2[f2_slot(N, T)], t.NC, c, f, m0, m1, nullptr);
}

// slot -> zone pair for the launches whose waves overlap by one slot: lane 0 of a wave repeats the last slot of the wave
// before it (it only hands its records to lane 1), lanes 1..63 own 63 new slots.  Same XCD-tiled row order as LinBox.
template <int WAVES = 4>
__device__ __forceinline__ void fold_thread(const LinBox& b, unsigned bid, int& i, int& j, int& k, bool& owner)
{
    if (b.ty > 0) {
        const unsigned per = b.nb >> 3;
        bid = (bid & 7u) * per + (bid >> 3);
    }
    const int lane = threadIdx.x & 63;
    const long total = (long)b.n[0] * b.n[1] * b.n[2];
    long sl = (long)(bid * (unsigned)WAVES + (threadIdx.x >> 6)) * 63 + lane - 1;
    owner = lane >= 1 && sl < total;
    if (sl < 0) sl = 0;
    if (sl >= total) sl = total - 1;
    const unsigned tid = (unsigned)sl;
    const unsigned ii = tid % (unsigned)b.n[0];
    const unsigned r = tid / (unsigned)b.n[0];
    i = b.lo[0] + b.w * (int)ii;
    if (b.ty > 0) {
        const unsigned rpt = (unsigned)b.ty * (unsigned)b.n[2];
        const unsigned yt = r / rpt;
        const unsigned rem = r - yt * rpt;
        const unsigned left = (unsigned)b.n[1] - yt * (unsigned)b.ty;
        const unsigned tyh = left < (unsigned)b.ty ? left : (unsigned)b.ty;
        const unsigned kk = rem / tyh;
        j = b.lo[1] + (int)(yt * (unsigned)b.ty + (rem - kk * tyh));
        k = b.lo[2] + (int)kk;
    } else {
        j = b.lo[1] + (int)(r % (unsigned)b.n[1]);
        k = b.lo[2] + (int)(r / (unsigned)b.n[1]);
    }
}

// k_trans1_fold_lds: the A records of a direction are parked in LDS (64 KB per workgroup, thread-private slots
// [face][zone][component][thread]): they are needed three times over the life of a direction and would cost 64 VGPRs held in
// registers (measured: 28 spilled at two waves per SIMD, break-even; profiles/EXPERIMENTS.md).
// FOLD_WG: threads per workgroup of that launch (a wave's 16 KB of slots are its own)
#ifndef FOLD_WG
#define FOLD_WG 256
#endif
// record (face f, zone w) of thread `th`
template <bool NOX = false>          // NOX: the species record was not parked (gamma_law_edges)
__device__ __forceinline__ void park_get(const double* __restrict__ park, int f, int w, int th, double r[NF1])
{
#pragma unroll
    for (int n = 0; n < NF1; ++n) {
        if (NOX && n == FX) { r[n] = 0.0; continue; }
        r[n] = park[((f * 2 + w) * NF1 + n) * FOLD_WG + th];
    }
}

// The waves of k_trans1_fold_lds overlap by one slot each (fold_thread: 63 new slots per wave): the only foreign slot a lane
// reads is its left neighbour's, in the same wave, and LDS is in order per wave -- no workgroup barrier, the waves of a CU run
// their load and compute phases independently (4.52 -> 4.39 ms against workgroups overlapping by one slot with __syncthreads,
// profiles/r03x_*).
#define FOLD_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                         __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
template <int T, int GEN, bool TX_HERE>
__device__ __forceinline__ void trans1_fold_dir_lds(const Tile& t, const int ijk[3], bool v1, bool owner, unsigned c,
                                                    const double* __restrict__ Q, const DevScratch& S, const DevGeom& g,
                                                    double cdtdt, double cdtdx, const DevParams& P, double* __restrict__ park,
                                                    const D2& c0)          // sound speeds of the thread's own zones
{
    constexpr int O = (T == 1) ? 2 : 1;
    const Str s = gstr(t);
    const unsigned st = dstr(s, T), so = dstr(s, O);
    const long NC = t.NC;
    const double* Cp = Q + PC * NC;
    const int th = threadIdx.x;

    FOLD_SYNC();                                   // the readers of the previous direction's records are done
    {
        double A[2][NF1];
        {
            double qm[2][NEDGE], qp[2][NEDGE];
            load_edge_2<gamma_law_edges(GEN)>(S.QM[T], NC, c, qm, 1.0 / (P.gamma - 1.0));
            load_edge_2<gamma_law_edges(GEN)>(S.QP[T], NC, c, qp, 1.0 / (P.gamma - 1.0));
            const D2 cl = ldg2(Cp, c - st), cr = c0;
            f1_solve_2<T, GEN>(qm, qp, cl, cr, wall_fac<T>(g, ijk[T]), P, A);
#pragma unroll
            for (int w = 0; w < 2; ++w)
#pragma unroll
                for (int n = 0; n < NF1; ++n) park[((0 * 2 + w) * NF1 + n) * FOLD_WG + th] = A[w][n];
            // the same edge states are the N = T states of the (T | x) combination, whose transverse flux F1[x] comes from
            // memory: done here, while they are in registers, instead of loading them a third time (trans1_fold_tx)
            if (TX_HERE) {
                bool in_t[2];
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    const int ix = ijk[0] + w;
                    in_t[w] = owner && ((w == 0) || v1) && ijk[T] >= t.lo[T] && ix >= t.lo[0] && ix <= t.hi[0];
                }
                if (in_t[0] || in_t[1]) {
                    double bnd[2];
                    bnd[0] = bnd[1] = wall_fac<T>(g, ijk[T]);
                    trans1_pair<T, 0, false, GEN>(t, S, c, st, 8u, qm, qp, cl, cr, bnd, cdtdx, in_t[0], in_t[1], P);
                }
            }
        }
        f1_at_2c<T, GEN>(t, S, g, P, c + st, ijk[T] + 1, c0, ldg2(Cp, c + st), A);
#pragma unroll
        for (int w = 0; w < 2; ++w)
#pragma unroll
            for (int n = 0; n < NF1; ++n) park[((1 * 2 + w) * NF1 + n) * FOLD_WG + th] = A[w][n];
    }
    FOLD_SYNC();

    const bool tin = owner && ijk[T] >= t.lo[T] && ijk[T] <= t.hi[T];
    double fr[NF1], fl[NF1];
    // ---- N = x
    {
        const bool m0 = tin && ijk[0] >= t.lo[0], m1 = tin && v1 && ijk[0] + 1 >= t.lo[0];
        if (m0 || m1) {
            double q[2][NEDGE], qmo[2][NEDGE], qpo[2][NEDGE];
            load_edge_2<gamma_law_edges(GEN)>(S.QM[0], NC, c, q, 1.0 / (P.gamma - 1.0));
            const int tl = th > 0 ? th - 1 : 0;    // thread 0 owns nothing
            park_get(park, 1, 1, tl, fr); park_get(park, 0, 1, tl, fl);
            trans_single<T>(q[0], fr, fl, P.gamma, cdtdt, P, qmo[0]);
            park_get(park, 1, 0, th, fr); park_get(park, 0, 0, th, fl);
            trans_single<T>(q[1], fr, fl, P.gamma, cdtdt, P, qmo[1]);
            load_edge_2<gamma_law_edges(GEN)>(S.QP[0], NC, c, q, 1.0 / (P.gamma - 1.0));
            trans_single<T>(q[0], fr, fl, P.gamma, cdtdt, P, qpo[0]);
            park_get(park, 1, 1, th, fr); park_get(park, 0, 1, th, fl);
            trans_single<T>(q[1], fr, fl, P.gamma, cdtdt, P, qpo[1]);
            const D2 cl = ldg2(Cp, c - 8u);
            double bnd[2] = { wall_fac<0>(g, ijk[0]), wall_fac<0>(g, ijk[0] + 1) };
            trans1_solve_store<0, T, GEN>(t, S, c, qmo, qpo, cl, c0, bnd, m0, m1, P);
        }
    }
    // ---- N = O
    {
        const bool m0 = tin && ijk[O] >= t.lo[O], m1 = m0 && v1;
        if (m0 || m1) {
            double q[2][NEDGE], qmo[2][NEDGE], qpo[2][NEDGE];
            const D2 cso = ldg2(Cp, c - so);       // sound speeds of the zones below: three uses
            {
                double B0[2][NF1], B1[2][NF1];
                f1_at_2c<T, GEN>(t, S, g, P, c - so, ijk[T], ldg2(Cp, c - so - st), cso, B0);
                f1_at_2c<T, GEN>(t, S, g, P, c - so + st, ijk[T] + 1, cso, ldg2(Cp, c - so + st), B1);
                load_edge_2<gamma_law_edges(GEN)>(S.QM[O], NC, c, q, 1.0 / (P.gamma - 1.0));
#pragma unroll
                for (int w = 0; w < 2; ++w) trans_single<T>(q[w], B1[w], B0[w], P.gamma, cdtdt, P, qmo[w]);
            }
            load_edge_2<gamma_law_edges(GEN)>(S.QP[O], NC, c, q, 1.0 / (P.gamma - 1.0));
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                park_get(park, 1, w, th, fr); park_get(park, 0, w, th, fl);
                trans_single<T>(q[w], fr, fl, P.gamma, cdtdt, P, qpo[w]);
            }
            double bnd[2];
            bnd[0] = bnd[1] = wall_fac<O>(g, ijk[O]);
            trans1_solve_store<O, T, GEN>(t, S, c, qmo, qpo, cso, c0, bnd, m0, m1, P);
        }
    }
}

// ---- the same with every phase's edge states requested one phase ahead (FOLD_REQUEST_AHEAD; the `contract` build's default-solver
// instantiation: its 5-variable edge states leave the ~40 registers a pending pair of edge states needs below the two-wave
// limit).  A wave's loads for the next phase are in flight while it solves the current one, instead of both waves of a SIMD
// waiting at the head of every phase.
#ifndef FOLD_REQUEST_AHEAD
#ifdef CAD_NUMERICS_CONTRACT
#define FOLD_REQUEST_AHEAD 1
#else
#define FOLD_REQUEST_AHEAD 0
#endif
#endif
struct EdgeReq { D2 m[NEDGE], p[NEDGE]; };       // requested minus / plus states of a face pair (slots PRE, PX stay untouched with NOPRE)

template <bool NOPRE>
__device__ __forceinline__ void edge_request(const double* __restrict__ EM, const double* __restrict__ EP, long NC, unsigned c, EdgeReq& r)
{
#pragma unroll
    for (int n = 0; n < NEDGE; ++n) {
        if (NOPRE && (n == PRE || n == PX)) continue;
        r.m[n] = ldg2(EM + (long)n * NC, c);
        r.p[n] = ldg2(EP + (long)n * NC, c);
    }
}

template <bool NOPRE>
__device__ __forceinline__ void edge_take(const D2 r[NEDGE], double q[2][NEDGE], double g1inv)
{
#pragma unroll
    for (int n = 0; n < NEDGE; ++n) {
        if (NOPRE && (n == PRE || n == PX)) continue;
        q[0][n] = r[n].a; q[1][n] = r[n].b;
    }
    if (NOPRE) { q[0][PRE] = q[0][PP] * g1inv; q[1][PRE] = q[1][PP] * g1inv; q[0][PX] = q[1][PX] = 1.0; }
}

template <int T, int GEN, bool TX_HERE>
__device__ __forceinline__ void trans1_fold_dir_ahead(const Tile& t, const int ijk[3], bool v1, bool owner, unsigned c,
                                                      const double* __restrict__ Q, const DevScratch& S, const DevGeom& g,
                                                      double cdtdt, double cdtdx, const DevParams& P, double* __restrict__ park,
                                                      const D2& c0)
{
    constexpr int O = (T == 1) ? 2 : 1;
    constexpr bool NP = gamma_law_edges(GEN);
    const Str s = gstr(t);
    const unsigned st = dstr(s, T), so = dstr(s, O);
    const long NC = t.NC;
    const double* Cp = Q + PC * NC;
    const int th = threadIdx.x;
    const double g1inv = 1.0 / (P.gamma - 1.0);

    FOLD_SYNC();                                   // the readers of the previous direction's records are done
    EdgeReq e0, e1;
    edge_request<NP>(S.QM[T], S.QP[T], NC, c, e0);
    const D2 cl = ldg2(Cp, c - st);
    edge_request<NP>(S.QM[T], S.QP[T], NC, c + st, e1);           // ahead: the faces above
    const D2 cst = ldg2(Cp, c + st);
    {
        double A[2][NF1];
        double qm[2][NEDGE], qp[2][NEDGE];
        edge_take<NP>(e0.m, qm, g1inv); edge_take<NP>(e0.p, qp, g1inv);
        f1_solve_2<T, GEN>(qm, qp, cl, c0, wall_fac<T>(g, ijk[T]), P, A);
#pragma unroll
        for (int w = 0; w < 2; ++w)
#pragma unroll
            for (int n = 0; n < NF1; ++n) { if (NP && n == FX) continue; park[((0 * 2 + w) * NF1 + n) * FOLD_WG + th] = A[w][n]; }   // no species record
        if (TX_HERE) {                             // the (T | x) combination on the same edge states (see trans1_fold_dir_lds)
            bool in_t[2];
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const int ix = ijk[0] + w;
                in_t[w] = owner && ((w == 0) || v1) && ijk[T] >= t.lo[T] && ix >= t.lo[0] && ix <= t.hi[0];
            }
            if (in_t[0] || in_t[1]) {
                double bnd[2];
                bnd[0] = bnd[1] = wall_fac<T>(g, ijk[T]);
                trans1_pair<T, 0, false, GEN>(t, S, c, st, 8u, qm, qp, cl, c0, bnd, cdtdx, in_t[0], in_t[1], P);
            }
        }
    }
    EdgeReq x0;
    edge_request<NP>(S.QM[0], S.QP[0], NC, c, x0);                // ahead: the x faces of the N = x phase
    const D2 clx = ldg2(Cp, c - 8u);
    {
        double A[2][NF1];
        double qm[2][NEDGE], qp[2][NEDGE];
        edge_take<NP>(e1.m, qm, g1inv); edge_take<NP>(e1.p, qp, g1inv);
        f1_solve_2<T, GEN>(qm, qp, c0, cst, wall_fac<T>(g, ijk[T] + 1), P, A);
#pragma unroll
        for (int w = 0; w < 2; ++w)
#pragma unroll
            for (int n = 0; n < NF1; ++n) { if (NP && n == FX) continue; park[((1 * 2 + w) * NF1 + n) * FOLD_WG + th] = A[w][n]; }
    }
    FOLD_SYNC();

    EdgeReq b0;
    edge_request<NP>(S.QM[T], S.QP[T], NC, c - so, b0);           // ahead: the T faces of the zones below (N = O phase)
    const D2 cso = ldg2(Cp, c - so), csom = ldg2(Cp, c - so - st), csop = ldg2(Cp, c - so + st);

    const bool tin = owner && ijk[T] >= t.lo[T] && ijk[T] <= t.hi[T];
    double fr[NF1], fl[NF1];
    // ---- N = x
    {
        const bool m0 = tin && ijk[0] >= t.lo[0], m1 = tin && v1 && ijk[0] + 1 >= t.lo[0];
        if (m0 || m1) {
            double q[2][NEDGE], qmo[2][NEDGE], qpo[2][NEDGE];
            edge_take<NP>(x0.m, q, g1inv);
            const int tl = th > 0 ? th - 1 : 0;    // thread 0 owns nothing
            park_get<NP>(park, 1, 1, tl, fr); park_get<NP>(park, 0, 1, tl, fl);
            trans_single<T>(q[0], fr, fl, P.gamma, cdtdt, P, qmo[0]);
            park_get<NP>(park, 1, 0, th, fr); park_get<NP>(park, 0, 0, th, fl);
            trans_single<T>(q[1], fr, fl, P.gamma, cdtdt, P, qmo[1]);
            edge_take<NP>(x0.p, q, g1inv);
            trans_single<T>(q[0], fr, fl, P.gamma, cdtdt, P, qpo[0]);
            park_get<NP>(park, 1, 1, th, fr); park_get<NP>(park, 0, 1, th, fl);
            trans_single<T>(q[1], fr, fl, P.gamma, cdtdt, P, qpo[1]);
            double bnd[2] = { wall_fac<0>(g, ijk[0]), wall_fac<0>(g, ijk[0] + 1) };
            trans1_solve_store<0, T, GEN>(t, S, c, qmo, qpo, clx, c0, bnd, m0, m1, P);
        }
    }
    // ---- N = O
    {
        const bool m0 = tin && ijk[O] >= t.lo[O], m1 = m0 && v1;
        if (m0 || m1) {
            double q[2][NEDGE], qmo[2][NEDGE], qpo[2][NEDGE];
            EdgeReq b1, o0;
            edge_request<NP>(S.QM[T], S.QP[T], NC, c - so + st, b1);      // ahead: the second pair of faces below
            {
                double B0[2][NF1], B1[2][NF1];
                {
                    double qm[2][NEDGE], qp[2][NEDGE];
                    edge_take<NP>(b0.m, qm, g1inv); edge_take<NP>(b0.p, qp, g1inv);
                    f1_solve_2<T, GEN>(qm, qp, csom, cso, wall_fac<T>(g, ijk[T]), P, B0);
                }
                edge_request<NP>(S.QM[O], S.QP[O], NC, c, o0);            // ahead: the O faces themselves
                {
                    double qm[2][NEDGE], qp[2][NEDGE];
                    edge_take<NP>(b1.m, qm, g1inv); edge_take<NP>(b1.p, qp, g1inv);
                    f1_solve_2<T, GEN>(qm, qp, cso, csop, wall_fac<T>(g, ijk[T] + 1), P, B1);
                }
                edge_take<NP>(o0.m, q, g1inv);
#pragma unroll
                for (int w = 0; w < 2; ++w) trans_single<T>(q[w], B1[w], B0[w], P.gamma, cdtdt, P, qmo[w]);
            }
            edge_take<NP>(o0.p, q, g1inv);
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                park_get<NP>(park, 1, w, th, fr); park_get<NP>(park, 0, w, th, fl);
                trans_single<T>(q[w], fr, fl, P.gamma, cdtdt, P, qpo[w]);
            }
            double bnd[2];
            bnd[0] = bnd[1] = wall_fac<O>(g, ijk[O]);
            trans1_solve_store<O, T, GEN>(t, S, c, qmo, qpo, cso, c0, bnd, m0, m1, P);
        }
    }
}

template <int GEN, bool LV = false>
__global__ void __launch_bounds__(FOLD_WG) CG_TWO_WAVES k_trans1_fold_lds(Tile t, LinBox b, const double* __restrict__ Q, DevScratch S, DevGeom g,
                                                         double cdtdx, double cdtdy, double cdtdz, DevParams P, LevelTab lv)
{
    __shared__ double park[2 * 2 * NF1 * FOLD_WG];
    DT_THIRDS_FROM_DEVICE();
    unsigned vb = blockIdx.x;
    if (LV) { const LevelBox& B = level_box(lv, vb); t = B.t; b = B.b[LB_FOLD]; S = B.S; Q = B.S.Q; }
    int ijk[3];
    bool owner;
    fold_thread<FOLD_WG / 64>(b, vb, ijk[0], ijk[1], ijk[2], owner);
    const bool v1 = ijk[0] + 1 <= b.hi0;
    const unsigned c = goff(t, ijk[0], ijk[1], ijk[2]);
    const D2 c0 = ldg2(Q + PC * t.NC, c);
    if (FOLD_REQUEST_AHEAD && gamma_law_edges(GEN)) {
        trans1_fold_dir_ahead<1, GEN, true>(t, ijk, v1, owner, c, Q, S, g, cdtdy, cdtdx, P, park, c0);
        trans1_fold_dir_ahead<2, GEN, true>(t, ijk, v1, owner, c, Q, S, g, cdtdz, cdtdx, P, park, c0);
    } else {
        trans1_fold_dir_lds<1, GEN, true>(t, ijk, v1, owner, c, Q, S, g, cdtdy, cdtdx, P, park, c0);
        trans1_fold_dir_lds<2, GEN, true>(t, ijk, v1, owner, c, Q, S, g, cdtdz, cdtdx, P, park, c0);
    }
}

// ---------------------------------------------------------------------------------------
// k_trans1_tile (round 5): the same stage with a (j,k) TILE of rows per workgroup, a WAVE per row.
//   k_trans1_fold_lds shares nothing between waves: of its 14 Riemann solves per zone pair, 6 repeat first-stage solves a
//   neighbouring row does too (the face above, and both faces of the zone below in the other transverse direction), and each
//   repetition re-reads its edge states.  Here the RY x RZ waves of a workgroup own RY x RZ rows of ONE run of 63 x-slots (every
//   wave load is still one contiguous 1-KB piece of a row -- the brick-shaped tile of round 4 lost on exactly that), every wave
//   solves the low y- and z-face of its row, the (RY+1)(RZ+1) - RY RZ face rows on the rim of the tile (the faces above it, and those
//   of the rows below it in the other direction) are dealt to the waves, and all first-stage records go through LDS in the 5-value
//   state form (rho, un, ut, utt, p): 2 x 15 face rows x 5 KB = 150 KB for the 4 x 2 tile, one workgroup of 8 waves per CU -- the
//   same two waves per SIMD as the fold kernel.  Per zone pair: 2 + 14/8 first-stage solves instead of 8, 6 second-stage solves as
//   before; ~110 vector loads instead of ~180.
//   Phases: (1) y first stage + (y|x); barrier; (2) z first stage + (z|x) + (z|y) on the z edge states it holds anyway; barrier;
//   (3) (x|y), (x|z) on one load of the x edge states, (y|z).
//   Slots: position p = 63 * workgroup + lane - 1 in the concatenation of the tiles' rows (a wave may straddle two tiles; all
//   waves of a workgroup straddle alike, so `lane` identifies the x-slot in every row); lane 0 repeats the slot before (fold_thread).
//   `contract` build, default solver set only (the 7-value records of the `exact` build do not fit the LDS of a CU).
// ---------------------------------------------------------------------------------------
struct TileRows { int lo[3]; int hi0; int nslot, ny, nz, ntj, ntk, band; unsigned nb; };
constexpr int NRQ = 5;                             // parked record: interface state (rho, un, ut, utt, p)

template <int RY, int RZ>
struct TileGeo {
    static constexpr int NW = RY * RZ, NFR = (RY + 1) * (RZ + 1), NEX = NFR - NW;
    // slot of the y-records of face row (j0 + a, k0 + b), a in [0, RY], b in [-1, RZ - 1]; of the z-records, a in [-1, RY - 1], b in [0, RZ]
    __host__ __device__ static constexpr int fy(int a, int b) { return (b + 1) * (RY + 1) + a; }
    __host__ __device__ static constexpr int fz(int a, int b) { return (a + 1) * (RZ + 1) + b; }
};

__device__ __forceinline__ void rec_put(double* __restrict__ L, int fr, int w, int lane, const IFlux& f)
{
    double* p = L + ((fr * 2 + w) * NRQ) * 64 + lane;
    p[0] = f.rho_g; p[64] = f.ugd; p[128] = f.ut; p[192] = f.utt; p[256] = f.pgd;
}
template <int T>
__device__ __forceinline__ void rec_get(const double* __restrict__ L, int fr, int w, int lane, double g1inv, double r[NF1])
{
    const double* p = L + ((fr * 2 + w) * NRQ) * 64 + lane;
    const double pg = p[256];
    qstate_to_rec<T>(p[0], p[64], p[128], p[192], pg, pg * g1inv, 1.0, r);
}

template <int D, int GEN>
__device__ __forceinline__ void f1_solve_2f(const double qm[2][NEDGE], const double qp[2][NEDGE], const D2& cl, const D2& cr,
                                            double bnd, const DevParams& P, IFlux f[2])
{
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        RState ql, qr;
        double Xl, Xr;
        rstate_from_edge<D>(qm[w], P.gamma, ql, Xl);
        rstate_from_edge<D>(qp[w], P.gamma, qr, Xr);
        interface_flux<D, GEN>(ql, qr, Xl, Xr, w ? cl.b : cl.a, w ? cr.b : cr.a, bnd, false, P, f[w]);
#ifndef TILE_NO_SCHED_BARRIER
        __builtin_amdgcn_sched_barrier(0);
#endif
    }
}

#ifdef CAD_NUMERICS_CONTRACT
#ifdef TILE_DIAG_NOBARRIER      // timing diagnostics (wrong results): no workgroup barriers / no rim-row solves
#define TILE_BARRIER() __builtin_amdgcn_wave_barrier()
#else
#define TILE_BARRIER() __syncthreads()
#endif
#ifdef TILE_DIAG_NORIM
#define TILE_RIM(x) false
#else
#define TILE_RIM(x) (x)
#endif
template <int GEN, int RY, int RZ>
__global__ void __launch_bounds__(64 * RY * RZ)
k_trans1_tile(Tile t, TileRows b, const double* __restrict__ Q, DevScratch S, DevGeom g,
              double cdtdx, double cdtdy, double cdtdz, DevParams P)
{
    using G = TileGeo<RY, RZ>;
    constexpr bool NP = gamma_law_edges(GEN);
    static_assert(NP, "k_trans1_tile parks 5-value records: gamma_law_edges instantiations only");
    __shared__ double rec[2 * G::NFR * 2 * NRQ * 64];
    double* const Ly = rec;
    double* const Lz = rec + G::NFR * 2 * NRQ * 64;
    DT_THIRDS_FROM_DEVICE();

    unsigned bid = blockIdx.x;
    bid = (bid & 7u) * (b.nb >> 3) + (bid >> 3);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // the wave index as a scalar
    const int jr = wave % RY, kr = wave / RY;
    const unsigned total = (unsigned)b.nslot * (unsigned)b.ntj * (unsigned)b.ntk;
    long pl = (long)bid * 63 + lane - 1;
    bool owner = lane >= 1 && pl < (long)total;
    if (pl < 0) pl = 0;
    if (pl >= (long)total) pl = (long)total - 1;
    const unsigned pos = (unsigned)pl;
    const unsigned tile = pos / (unsigned)b.nslot;
    const int xs = (int)(pos - tile * (unsigned)b.nslot);
    // tiles band by band in j (b.band tiles), k-plane by k-plane inside a band: the rows an XCD works on at one time are neighbours
    const unsigned per_band = (unsigned)b.band * (unsigned)b.ntk;
    const unsigned bd = tile / per_band;
    const unsigned rem = tile - bd * per_band;
    const unsigned left = (unsigned)b.ntj - bd * (unsigned)b.band;
    const unsigned bw = left < (unsigned)b.band ? left : (unsigned)b.band;
    const unsigned tk = rem / bw;
    const unsigned tj = bd * (unsigned)b.band + (rem - tk * bw);
    const int j0 = b.lo[1] + (int)tj * RY, k0 = b.lo[2] + (int)tk * RZ;
    const int hj = b.lo[1] + b.ny - 1, hk = b.lo[2] + b.nz - 1;          // last rows of the launch box
    int ijk[3];
    ijk[0] = b.lo[0] + 2 * xs;
    ijk[1] = j0 + jr;
    ijk[2] = k0 + kr;
    if (ijk[1] > hj || ijk[2] > hk) owner = false;                     // a tile may reach past the box: such a row repeats the last one
    if (ijk[1] > hj) ijk[1] = hj;
    if (ijk[2] > hk) ijk[2] = hk;
    const bool v1 = ijk[0] + 1 <= b.hi0;
    const unsigned c = goff(t, ijk[0], ijk[1], ijk[2]);
    const Str s = gstr(t);
    const long NC = t.NC;
    const double* Cp = Q + PC * NC;
    const double g1inv = 1.0 / (P.gamma - 1.0);
    const D2 c0 = ldg2(Cp, c);
    const bool tin_y = owner && ijk[1] >= t.lo[1] && ijk[1] <= t.hi[1];
    const bool tin_z = owner && ijk[2] >= t.lo[2] && ijk[2] <= t.hi[2];
    double fr[NF1], fl[NF1];

    // ---- phase 1: first y solves (own low face, one rim face row per wave), (y|x)
    {
        EdgeReq e0, e1;
        edge_request<NP>(S.QM[1], S.QP[1], NC, c, e0);
        const D2 cl = ldg2(Cp, c - s.y);
        const int ex = wave;                                          // rim rows 0 .. NEX-1 go to waves 0 .. NEX-1
        const bool has_ex = TILE_RIM(ex < G::NEX);
        const int ea = ex < RZ ? RY : ex - RZ, eb = ex < RZ ? ex : -1;
        int jf = j0 + ea, kf = k0 + eb;
        if (jf > hj + 1) jf = hj + 1;
        if (kf > hk) kf = hk;
        const unsigned cfe = goff(t, ijk[0], jf, kf);
        D2 cle, cre;
        if (has_ex) { edge_request<NP>(S.QM[1], S.QP[1], NC, cfe, e1); cle = ldg2(Cp, cfe - s.y); cre = ldg2(Cp, cfe); }
        {
            double qm[2][NEDGE], qp[2][NEDGE];
            IFlux f[2];
            edge_take<NP>(e0.m, qm, g1inv); edge_take<NP>(e0.p, qp, g1inv);
            f1_solve_2f<1, GEN>(qm, qp, cl, c0, wall_fac<1>(g, ijk[1]), P, f);
            rec_put(Ly, G::fy(jr, kr), 0, lane, f[0]);
            rec_put(Ly, G::fy(jr, kr), 1, lane, f[1]);
            bool in_t[2];
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const int ix = ijk[0] + w;
                in_t[w] = owner && ((w == 0) || v1) && ijk[1] >= t.lo[1] && ix >= t.lo[0] && ix <= t.hi[0];
            }
            if (in_t[0] || in_t[1]) {
                double bnd[2];
                bnd[0] = bnd[1] = wall_fac<1>(g, ijk[1]);
                trans1_pair<1, 0, false, GEN>(t, S, c, s.y, 8u, qm, qp, cl, c0, bnd, cdtdx, in_t[0], in_t[1], P);
            }
        }
        if (has_ex) {
            double qm[2][NEDGE], qp[2][NEDGE];
            IFlux f[2];
            edge_take<NP>(e1.m, qm, g1inv); edge_take<NP>(e1.p, qp, g1inv);
            f1_solve_2f<1, GEN>(qm, qp, cle, cre, wall_fac<1>(g, jf), P, f);
            rec_put(Ly, G::fy(ea, eb), 0, lane, f[0]);
            rec_put(Ly, G::fy(ea, eb), 1, lane, f[1]);
        }
    }
#ifndef TILE_NO_PREFETCH
    // the first loads of a phase are requested in front of the barrier that opens it: no wave waits for memory behind a barrier
    EdgeReq ez0;
    edge_request<NP>(S.QM[2], S.QP[2], NC, c, ez0);
    const D2 clz0 = ldg2(Cp, c - s.z);
#endif
    TILE_BARRIER();

    // ---- phase 2: first z solves (own low face, rim rows from the last wave down), (z|x), (z|y)
    EdgeReq x0;
    D2 clx;
    {
#ifndef TILE_NO_PREFETCH
        EdgeReq e1;
        EdgeReq& e0 = ez0;
        const D2 cl = clz0;
#else
        EdgeReq e0, e1;
        edge_request<NP>(S.QM[2], S.QP[2], NC, c, e0);
        const D2 cl = ldg2(Cp, c - s.z);
#endif
        const int ex = G::NW - 1 - wave;
        const bool has_ex = TILE_RIM(ex < G::NEX);
        const int ea = ex < RY ? ex : -1, eb = ex < RY ? RZ : ex - RY;
        int jf = j0 + ea, kf = k0 + eb;
        if (jf > hj) jf = hj;
        if (kf > hk + 1) kf = hk + 1;
        const unsigned cfe = goff(t, ijk[0], jf, kf);
        D2 cle, cre;
        {
            double qm[2][NEDGE], qp[2][NEDGE];
            IFlux f[2];
            edge_take<NP>(e0.m, qm, g1inv); edge_take<NP>(e0.p, qp, g1inv);
            f1_solve_2f<2, GEN>(qm, qp, cl, c0, wall_fac<2>(g, ijk[2]), P, f);
            rec_put(Lz, G::fz(jr, kr), 0, lane, f[0]);
            rec_put(Lz, G::fz(jr, kr), 1, lane, f[1]);
            bool in_t[2];
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const int ix = ijk[0] + w;
                in_t[w] = owner && ((w == 0) || v1) && ijk[2] >= t.lo[2] && ix >= t.lo[0] && ix <= t.hi[0];
            }
            double bnd[2];
            bnd[0] = bnd[1] = wall_fac<2>(g, ijk[2]);
            if (in_t[0] || in_t[1])
                trans1_pair<2, 0, false, GEN>(t, S, c, s.z, 8u, qm, qp, cl, c0, bnd, cdtdx, in_t[0], in_t[1], P);
            // ahead: the rim row (requested here, not earlier: the z edge states stay live across (z|x) for (z|y))
            if (has_ex) { edge_request<NP>(S.QM[2], S.QP[2], NC, cfe, e1); cle = ldg2(Cp, cfe - s.z); cre = ldg2(Cp, cfe); }
            // (z|y): the z edge states corrected with the y fluxes of the zones below (minus) and of the own zones (plus)
            const bool m0 = tin_y && ijk[2] >= t.lo[2], m1 = m0 && v1;
            if (m0 || m1) {
                double qmo[2][NEDGE], qpo[2][NEDGE];
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    rec_get<1>(Ly, G::fy(jr + 1, kr - 1), w, lane, g1inv, fr); rec_get<1>(Ly, G::fy(jr, kr - 1), w, lane, g1inv, fl);
                    trans_single<1>(qm[w], fr, fl, P.gamma, cdtdy, P, qmo[w]);
                    rec_get<1>(Ly, G::fy(jr + 1, kr), w, lane, g1inv, fr); rec_get<1>(Ly, G::fy(jr, kr), w, lane, g1inv, fl);
                    trans_single<1>(qp[w], fr, fl, P.gamma, cdtdy, P, qpo[w]);
                }
                trans1_solve_store<2, 1, GEN>(t, S, c, qmo, qpo, cl, c0, bnd, m0, m1, P);
            }
        }
        if (has_ex) {
            double qm[2][NEDGE], qp[2][NEDGE];
            IFlux f[2];
            edge_take<NP>(e1.m, qm, g1inv); edge_take<NP>(e1.p, qp, g1inv);
#ifndef TILE_NO_PREFETCH
            edge_request<NP>(S.QM[0], S.QP[0], NC, c, x0); clx = ldg2(Cp, c - 8u);      // ahead of the barrier, behind the rim request
#endif
            f1_solve_2f<2, GEN>(qm, qp, cle, cre, wall_fac<2>(g, kf), P, f);
            rec_put(Lz, G::fz(ea, eb), 0, lane, f[0]);
            rec_put(Lz, G::fz(ea, eb), 1, lane, f[1]);
        }
#ifndef TILE_NO_PREFETCH
        if (!has_ex) { edge_request<NP>(S.QM[0], S.QP[0], NC, c, x0); clx = ldg2(Cp, c - 8u); }
#endif
    }
    TILE_BARRIER();

    // ---- phase 3: (x|y) and (x|z) on one load of the x edge states, then (y|z)
    {
        EdgeReq y0;
#ifdef TILE_NO_PREFETCH
        edge_request<NP>(S.QM[0], S.QP[0], NC, c, x0);
        clx = ldg2(Cp, c - 8u);
#endif
        const int tl = lane > 0 ? lane - 1 : 0;                         // lane 0 owns nothing
        const bool x0ok = ijk[0] >= t.lo[0], x1ok = v1 && ijk[0] + 1 >= t.lo[0];
        double bndx[2] = { wall_fac<0>(g, ijk[0]), wall_fac<0>(g, ijk[0] + 1) };
        double qxm[2][NEDGE], qxp[2][NEDGE];
        edge_take<NP>(x0.m, qxm, g1inv); edge_take<NP>(x0.p, qxp, g1inv);
        if (tin_y && (x0ok || x1ok)) {
            double qmo[2][NEDGE], qpo[2][NEDGE];
            rec_get<1>(Ly, G::fy(jr + 1, kr), 1, tl, g1inv, fr); rec_get<1>(Ly, G::fy(jr, kr), 1, tl, g1inv, fl);
            trans_single<1>(qxm[0], fr, fl, P.gamma, cdtdy, P, qmo[0]);
            rec_get<1>(Ly, G::fy(jr + 1, kr), 0, lane, g1inv, fr); rec_get<1>(Ly, G::fy(jr, kr), 0, lane, g1inv, fl);
            trans_single<1>(qxm[1], fr, fl, P.gamma, cdtdy, P, qmo[1]);
            trans_single<1>(qxp[0], fr, fl, P.gamma, cdtdy, P, qpo[0]);
            rec_get<1>(Ly, G::fy(jr + 1, kr), 1, lane, g1inv, fr); rec_get<1>(Ly, G::fy(jr, kr), 1, lane, g1inv, fl);
            trans_single<1>(qxp[1], fr, fl, P.gamma, cdtdy, P, qpo[1]);
            trans1_solve_store<0, 1, GEN>(t, S, c, qmo, qpo, clx, c0, bndx, x0ok, x1ok, P);
        }
        edge_request<NP>(S.QM[1], S.QP[1], NC, c, y0);               // ahead: the y faces of (y|z)
        const D2 cly = ldg2(Cp, c - s.y);
        if (tin_z && (x0ok || x1ok)) {
            double qmo[2][NEDGE], qpo[2][NEDGE];
            rec_get<2>(Lz, G::fz(jr, kr + 1), 1, tl, g1inv, fr); rec_get<2>(Lz, G::fz(jr, kr), 1, tl, g1inv, fl);
            trans_single<2>(qxm[0], fr, fl, P.gamma, cdtdz, P, qmo[0]);
            rec_get<2>(Lz, G::fz(jr, kr + 1), 0, lane, g1inv, fr); rec_get<2>(Lz, G::fz(jr, kr), 0, lane, g1inv, fl);
            trans_single<2>(qxm[1], fr, fl, P.gamma, cdtdz, P, qmo[1]);
            trans_single<2>(qxp[0], fr, fl, P.gamma, cdtdz, P, qpo[0]);
            rec_get<2>(Lz, G::fz(jr, kr + 1), 1, lane, g1inv, fr); rec_get<2>(Lz, G::fz(jr, kr), 1, lane, g1inv, fl);
            trans_single<2>(qxp[1], fr, fl, P.gamma, cdtdz, P, qpo[1]);
            trans1_solve_store<0, 2, GEN>(t, S, c, qmo, qpo, clx, c0, bndx, x0ok, x1ok, P);
        }
        // (y|z): the y edge states corrected with the z fluxes of the zones below in y (minus) and of the own zones (plus)
        const bool m0 = tin_z && ijk[1] >= t.lo[1], m1 = m0 && v1;
        if (m0 || m1) {
            double q[2][NEDGE], qmo[2][NEDGE], qpo[2][NEDGE];
            edge_take<NP>(y0.m, q, g1inv);
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                rec_get<2>(Lz, G::fz(jr - 1, kr + 1), w, lane, g1inv, fr); rec_get<2>(Lz, G::fz(jr - 1, kr), w, lane, g1inv, fl);
                trans_single<2>(q[w], fr, fl, P.gamma, cdtdz, P, qmo[w]);
            }
            edge_take<NP>(y0.p, q, g1inv);
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                rec_get<2>(Lz, G::fz(jr, kr + 1), w, lane, g1inv, fr); rec_get<2>(Lz, G::fz(jr, kr), w, lane, g1inv, fl);
                trans_single<2>(q[w], fr, fl, P.gamma, cdtdz, P, qpo[w]);
            }
            double bnd[2];
            bnd[0] = bnd[1] = wall_fac<1>(g, ijk[1]);
            trans1_solve_store<1, 2, GEN>(t, S, c, qmo, qpo, cly, c0, bnd, m0, m1, P);
        }
    }
}
#endif

// All three normal directions in one launch over grow(bx, 1): each F1 record is then fetched from HBM by one
// kernel instead of two (F1[T] serves the two N != T), the other reads hit in L2.
template <bool RE, int NMASK = 7, int GEN = 2>
__global__ void __launch_bounds__(256) CG_TWO_WAVES k_trans1(Tile t, LinBox b, const double* __restrict__ Q, DevScratch S, DevGeom g,
                                                double cdtdx, double cdtdy, double cdtdz, DevParams P)
{
    int ijk[3];
    if (!box_thread(b, ijk[0], ijk[1], ijk[2])) return;
    DT_THIRDS_FROM_DEVICE();
    const bool v1 = ijk[0] + 1 <= b.hi0;          // second zone of the pair inside the box
    const unsigned c = goff(t, ijk[0], ijk[1], ijk[2]);
    if (NMASK & 1) trans1_body<0, RE, GEN>(t, ijk, v1, c, Q, S, g, cdtdy, cdtdz, P);
    if (NMASK & 2) trans1_body<1, RE, GEN>(t, ijk, v1, c, Q, S, g, cdtdx, cdtdz, P);
    if (NMASK & 4) trans1_body<2, RE, GEN>(t, ijk, v1, c, Q, S, g, cdtdx, cdtdy, P);
}

// one normal direction of the final stage for the faces (ijk) and (ijk + x); v0 / v1: the faces belong to
// nodal(bx, N)
// c0 / c1: compute face 0 / 1 of the pair; v0 / v1: store its outputs (fluxes, mass_fluxes, qe and, with STORE_FL, the
// record for consup).  R returns the records of both faces.
template <int N, bool RE, bool LIM, bool STORE_FL = true, int GEN = 2>
__device__ __forceinline__ void final_body(const Tile& t, const int ijk[3], bool v0, bool v1, unsigned c,
                                           const double* __restrict__ Q, const DevScratch& S, const DevGeom& g,
                                           const DFab& U, const DFab& fluxes, const DFab& mass, const DFab& qe,
                                           double hdtdx_t1, double hdtdx_t2, double dt, double area, double dxn,
                                           int acc_hi, int assign, const DevParams& P, double R[2][NFIN])
{
    constexpr int T1 = (N == 0) ? 1 : 0;
    constexpr int T2 = (N == 2) ? 1 : 2;
    if (STORE_FL && !v0 && !v1) return;
    const Str s = gstr(t);
    const unsigned sn = dstr(s, N), s1 = dstr(s, T1), s2 = dstr(s, T2);
    const long NC = t.NC;

    double q[2][NEDGE], ql[2][NEDGE], qr[2][NEDGE];
    double f1r[2][NF1], f1l[2][NF1], f2r[2][NF1], f2l[2][NF1];
    const double* F12 = S.F2[f2_slot(T1, T2)];   // F^{T1|T2}: flux_t1
    const double* F21 = S.F2[f2_slot(T2, T1)];   // F^{T2|T1}: flux_t2

    // minus states (zones c - sn)
    load_edge_2<gamma_law_edges(GEN)>(S.QM[N], NC, c, q, 1.0 / (P.gamma - 1.0));
    if (RE && P.ppm_temp_fix == 2 && P.riemann_solver != 2) { temp_fix_edge(q[0], P); temp_fix_edge(q[1], P); }   // changed by its first solve
#ifdef DIAG_F2_REUSE      // timing diagnostic (wrong results): two record loads per face pair instead of eight
    load_f1_2<T1, (kQI && GEN == 0)>(F12, NC, c, f1l);
    load_f1_2<T2, (kQI && GEN == 0)>(F21, NC, c, f2l);
#pragma unroll
    for (int w = 0; w < 2; ++w)
#pragma unroll
        for (int n = 0; n < NF1; ++n) { f1r[w][n] = f1l[w][n] * 1.01; f2r[w][n] = f2l[w][n] * 0.99; }
#else
    load_f1_2<T1, (kQI && GEN == 0)>(F12, NC, c - sn + s1, f1r);
    load_f1_2<T1, (kQI && GEN == 0)>(F12, NC, c - sn, f1l);
    load_f1_2<T2, (kQI && GEN == 0)>(F21, NC, c - sn + s2, f2r);
    load_f1_2<T2, (kQI && GEN == 0)>(F21, NC, c - sn, f2l);
#endif
    if (RE && P.reset_rhoe == 1) {                 // transverse_reset_rhoe = 1: the (rho e) flux differences as well
        const double* E12 = S.F2E[f2_slot(T1, T2)];
        const double* E21 = S.F2E[f2_slot(T2, T1)];
        const D2 e1r = ldg2(E12, c - sn + s1), e1l = ldg2(E12, c - sn), e2r = ldg2(E21, c - sn + s2), e2l = ldg2(E21, c - sn);
        trans_final(q[0], f1r[0], f1l[0], f2r[0], f2l[0], P.gamma, hdtdx_t1, hdtdx_t2, P, ql[0], e1r.a, e1l.a, e2r.a, e2l.a);
        trans_final(q[1], f1r[1], f1l[1], f2r[1], f2l[1], P.gamma, hdtdx_t1, hdtdx_t2, P, ql[1], e1r.b, e1l.b, e2r.b, e2l.b);
    } else {
#pragma unroll
        for (int w = 0; w < 2; ++w) trans_final(q[w], f1r[w], f1l[w], f2r[w], f2l[w], P.gamma, hdtdx_t1, hdtdx_t2, P, ql[w]);
    }

    // plus states (zones c)
    load_edge_2<gamma_law_edges(GEN)>(S.QP[N], NC, c, q, 1.0 / (P.gamma - 1.0));
    if (RE && P.ppm_temp_fix == 2 && P.riemann_solver != 2) { temp_fix_edge(q[0], P); temp_fix_edge(q[1], P); }
#ifndef DIAG_F2_REUSE
    load_f1_2<T1, (kQI && GEN == 0)>(F12, NC, c + s1, f1r);
    load_f1_2<T1, (kQI && GEN == 0)>(F12, NC, c, f1l);
    load_f1_2<T2, (kQI && GEN == 0)>(F21, NC, c + s2, f2r);
    load_f1_2<T2, (kQI && GEN == 0)>(F21, NC, c, f2l);
#endif
    if (RE && P.reset_rhoe == 1) {
        const double* E12 = S.F2E[f2_slot(T1, T2)];
        const double* E21 = S.F2E[f2_slot(T2, T1)];
        const D2 e1r = ldg2(E12, c + s1), e1l = ldg2(E12, c), e2r = ldg2(E21, c + s2), e2l = ldg2(E21, c);
        trans_final(q[0], f1r[0], f1l[0], f2r[0], f2l[0], P.gamma, hdtdx_t1, hdtdx_t2, P, qr[0], e1r.a, e1l.a, e2r.a, e2l.a);
        trans_final(q[1], f1r[1], f1l[1], f2r[1], f2l[1], P.gamma, hdtdx_t1, hdtdx_t2, P, qr[1], e1r.b, e1l.b, e2r.b, e2l.b);
    } else {
#pragma unroll
        for (int w = 0; w < 2; ++w) trans_final(q[w], f1r[w], f1l[w], f2r[w], f2l[w], P.gamma, hdtdx_t1, hdtdx_t2, P, qr[w]);
    }

    // lazy_av: requested here and reduced to two values before the Riemann solves, so that the chain div(u) -> predicate -> old
    // state does not lengthen the tail on a compressive flow
    double div1[2];
    if (lazy_av<LIM>()) av_div1(S, c, s1, s2, P, div1);
    const D2 cl = ldg2(Q + PC * NC, c - sn);
    const D2 cr = ldg2(Q + PC * NC, c);
    const unsigned usn = 8u * (N == 0 ? 1u : N == 1 ? (unsigned)U.sy : (unsigned)U.sz);

    if (RE && P.ppm_temp_fix == 2 && P.riemann_solver != 2) {
#pragma unroll
        for (int w = 0; w < 2; ++w) { temp_fix_edge(ql[w], P); temp_fix_edge(qr[w], P); }
    }
    IFlux f[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        RState rl, rr;
        double Xl, Xr;
        rstate_from_edge<N>(ql[w], P.gamma, rl, Xl);
        rstate_from_edge<N>(qr[w], P.gamma, rr, Xr);
        const int idxN = (N == 0) ? ijk[0] + w : ijk[N];
        interface_flux<N, GEN>(rl, rr, Xl, Xr, w ? cl.b : cl.a, w ? cr.b : cr.a, wall_fac<N>(g, idxN),
                          face_shock(S, P, c + 8u * w, sn), P, f[w]);
    }
    if (!lazy_av<LIM>()) av_div1(S, c, s1, s2, P, div1);
    // assign: bit 0 = assign (else accumulate) the fluxes, bits 1 and 2 = the two lazy loads (assign_word)
    final_flux_tail<N, LIM, (gamma_law_edges(GEN) && !LIM)>(t, S, f, c, s1, s2, U, foff(U, ijk[0], ijk[1], ijk[2]), usn, fluxes, mass, qe,
                            ijk[0], ijk[1], ijk[2], dt, area, dxn, g.dx[0] * g.dx[1] * g.dx[2], acc_hi, (assign & 1) != 0, lazy_av_on(assign),
                            div1, v0, v1, P, R);
    if (!STORE_FL) return;
    double* FL = S.FL[N];
    constexpr bool NOX = gamma_law_edges(GEN) && !LIM;      // record GX == record GRHO: not stored, consup reads GRHO
    if (v0 && v1) {
#pragma unroll
        for (int n = 0; n < NFIN; ++n) { if (NOX && n == GX) continue; stg2(FL + (long)n * NC, c, R[0][n], R[1][n]); }
    } else if (v0) {
#pragma unroll
        for (int n = 0; n < NFIN; ++n) { if (NOX && n == GX) continue; stg(FL + (long)n * NC, c, R[0][n]); }
    } else {
#pragma unroll
        for (int n = 0; n < NFIN; ++n) { if (NOX && n == GX) continue; stg(FL + (long)n * NC, c + 8u, R[1][n]); }
    }
}

// One launch per normal direction.  (All three in one launch, which fetches Sborder and div(u) once instead of
// three times, measured slower: 5.0 vs 4.6 ms at 256^3 -- ~150 concurrent streams per workgroup.)
template <int N, bool RE, bool LIM, int GEN = 2, bool LV = false>
__global__ void __launch_bounds__(256) CG_TWO_WAVES k_final(Tile t, LinBox b, const double* __restrict__ Q, DevScratch S, DevGeom g,
                                               DFab U, DFab fluxes, DFab mass, DFab qe,
                                               double hdtdx_t1, double hdtdx_t2, double dt, double area, double dxn,
                                               int acc_hi, int assign, DevParams P, LevelTab lv)
{
    RETURN_IF_BATCH_FAILED();
    unsigned vb = blockIdx.x;
    if (LV) {
        const LevelBox& B = level_box(lv, vb);
        t = B.t; b = B.b[N == 1 ? LB_FY : LB_FZ]; S = B.S; Q = B.S.Q; U = B.U; fluxes = B.fl[N]; mass = B.mass[N]; qe = B.qe[N]; acc_hi = B.acc_hi[N];
    }
    int ijk[3];
    if (!box_thread_at(b, vb, threadIdx.x, ijk[0], ijk[1], ijk[2])) return;
    if (P.dtp) {                                  // hdtdx = 0.5*dt/dx as on the host
        constexpr int T1 = (N == 0) ? 1 : 0, T2 = (N == 2) ? 1 : 2;
        dt = P.dtp[6];
        hdtdx_t1 = 0.5 * dt / g.dx[T1];
        hdtdx_t2 = 0.5 * dt / g.dx[T2];
    }
    const bool v1 = ijk[0] + 1 <= b.hi0;          // second face of the pair inside the box
    const unsigned c = goff(t, ijk[0], ijk[1], ijk[2]);
    double R[2][NFIN];
    final_body<N, RE, LIM, true, GEN>(t, ijk, true, v1, c, Q, S, g, U, fluxes, mass, qe, hdtdx_t1, hdtdx_t2, dt, area, dxn, acc_hi, assign, P, R);
}

// ---------------------------------------------------------------------------------------
// Castro::consup_hydro (Source/hydro/Castro_ctu.cpp:11-86), 3-D Cartesian
// ---------------------------------------------------------------------------------------
// CLEAN: the post-update sequence of do_advance_ctu fused in (Castro_advance_ctu.cpp:168-225, 386):
// raw minimum density, clean_state `ntimes` times, CFL time step of the cleaned zone, both minima
// reduced into red[0..1] (see castro_amd_clean_state_reduce_fab).
template <bool CLEAN>
__global__ void __launch_bounds__(256) k_consup(Tile t, LinBox b, DevScratch S, DFab Uin, DFab Unew, double dt,
                                                double area0, double area1, double area2, double vol,
                                                int from_sborder, DevParams P, int ntimes,
                                                double dx0, double dx1, double dx2, double* red)
{
    RETURN_IF_BATCH_FAILED();
    if (P.dtp) dt = P.dtp[6];
    int i, j, k;
    const bool valid = box_thread(b, i, j, k);
    double dtmin = 1.e200, rmin_raw = 1.e300, dtmin1 = 1.e200;
    if (valid) {
    const unsigned c = goff(t, i, j, k);
    const Str s = gstr(t);
    const unsigned sx = s.x, sy = s.y, sz = s.z;
    const long NC = t.NC;
    const double volinv = 1.0 / vol;
    const double* F0 = S.FL[0];
    const double* F1 = S.FL[1];
    const double* F2 = S.FL[2];
    const unsigned cn = foff(Unew, i, j, k);
    const unsigned ci = foff(Uin, i, j, k);

    // record index of conserved component m in the FL arrays
    constexpr int rec[NUM_STATE] = { GRHO, GMX, GMY, GMZ, GE, GEI, -1, GX };
    double un[NUM_STATE];

#pragma unroll
    for (int m = 0; m < NUM_STATE; ++m) {
        double* dst = Unew.p + m * Unew.sn;
        double u0 = from_sborder ? ldg(Uin.p + m * Uin.sn, ci) : ldg(dst, cn);
        if (m == UTEMP) {
            // zero flux: U + dt*(0)*volinv == U
            un[m] = u0;
            continue;
        }
        const long r = (long)rec[m] * NC;
        double unew = u0 + dt *
            ( ldg(F0 + r, c) * area0
            - ldg(F0 + r, c + sx) * area0
            + ldg(F1 + r, c) * area1
            - ldg(F1 + r, c + sy) * area1
            + ldg(F2 + r, c) * area2
            - ldg(F2 + r, c + sz) * area2
            ) * volinv;

        if (m == UEINT) {
            double pdu = (ldg(F0 + GPG * NC, c + sx) + ldg(F0 + GPG * NC, c)) *
                (ldg(F0 + GUG * NC, c + sx) * area0 - ldg(F0 + GUG * NC, c) * area0);

            pdu += (ldg(F1 + GPG * NC, c + sy) + ldg(F1 + GPG * NC, c)) *
                (ldg(F1 + GUG * NC, c + sy) * area1 - ldg(F1 + GUG * NC, c) * area1);

            pdu += (ldg(F2 + GPG * NC, c + sz) + ldg(F2 + GPG * NC, c)) *
                (ldg(F2 + GUG * NC, c + sz) * area2 - ldg(F2 + GUG * NC, c) * area2);

            pdu = 0.5 * pdu * volinv;

            unew = unew - dt * pdu;
        }
        un[m] = unew;
    }

    if (CLEAN) {
        rmin_raw = nan_guard(un[URHO]);
        clean_zone_dt(P, ntimes, dx0, dx1, dx2, un[URHO], un[UMX], un[UMY], un[UMZ], un[UEDEN], un[UEINT], un[UTEMP], un[UFS], dtmin1, dtmin);
    }
#pragma unroll
    for (int m = 0; m < NUM_STATE; ++m) {
        if (m == UTEMP && !CLEAN && !from_sborder) continue;     // unchanged in place
        stg(Unew.p + m * Unew.sn, cn, un[m]);
    }
    }
    if (CLEAN && red) wave_min3_atomic(dtmin, rmin_raw, dtmin1, red);      // per wave: any workgroup size (CASTRO_AMD_WG)
}

// ---------------------------------------------------------------------------------------
// k_final<x> and consup_hydro in one kernel: the x fluxes of a zone never leave the chip.
//   A thread owns the x-faces (i, i+1) like k_final<0> and the zones (i, i+1): their low x fluxes are its own two
//   records, the high flux of zone i+1 is the first record of the NEXT lane (one wave shuffle per component).  So that
//   no zone straddles two wavefronts, consecutive waves overlap by one slot: a wave advances 63 slots and its lane 63
//   only repeats the first slot of the next wave (1.6 % redundant solves, no LDS, no barrier).  A row of nx zones has
//   ceil(nx/2) zone slots and one more for the face hi+1.  The y and z flux records come from FL[1], FL[2], which
//   k_final<1>, k_final<2> have written before this launch.  Saves, per zone and step: FL[0] written and read (18
//   plane passes), Sborder read once instead of twice, one launch.
// ---------------------------------------------------------------------------------------
template <bool LIM, bool CLEAN, int GEN = 2, bool LV = false>
__global__ void __launch_bounds__(256) CG_TWO_WAVES k_finalx_consup(Tile t, XRows b, const double* __restrict__ Q, DevScratch S, DevGeom g,
                                                       DFab U, DFab fluxes, DFab mass, DFab qe, DFab Unew,
                                                       double hdtdy, double hdtdz, double dt,
                                                       double area0, double area1, double area2, double vol,
                                                       int acc_hi, int assign, int from_sborder, DevParams P, int ntimes,
                                                       double* red, LevelTab lv)
{
    RETURN_IF_BATCH_FAILED();
    if (P.dtp) { dt = P.dtp[6]; hdtdy = 0.5 * dt / g.dx[1]; hdtdz = 0.5 * dt / g.dx[2]; }
    unsigned bid = blockIdx.x;
    if (LV) {
        const LevelBox& B = level_box(lv, bid);
        t = B.t; b = B.xr; S = B.S; Q = B.S.Q; U = B.U; fluxes = B.fl[0]; mass = B.mass[0]; qe = B.qe[0]; Unew = B.Unew; acc_hi = B.acc_hi[0];
    }
    bid = (bid & 7u) * (b.nb >> 3) + (bid >> 3);
    const int lane = threadIdx.x & 63;
    const unsigned total = (unsigned)b.nslot * (unsigned)b.ny * (unsigned)b.nz;
    unsigned sl = (bid * b.wv + (threadIdx.x >> 6)) * 63u + (unsigned)lane;
    const bool live = sl < total;
    if (!live) sl = total - 1u;                       // keeps every lane inside the arrays; it stores nothing
    const unsigned row = sl / (unsigned)b.nslot;
    const int p = (int)(sl - row * (unsigned)b.nslot);
    int ijk[3];
    ijk[0] = b.lo[0] + 2 * p;
    if (b.ty > 0) {
        // rows y-tile by y-tile, z-plane by z-plane inside a tile (like LinBox): the y and z neighbours of the rows an
        // XCD works on at one time stay in its L2
        const unsigned rpt = (unsigned)b.ty * (unsigned)b.nz;
        const unsigned yt = row / rpt;
        const unsigned rem = row - yt * rpt;
        const unsigned left = (unsigned)b.ny - yt * (unsigned)b.ty;
        const unsigned tyh = left < (unsigned)b.ty ? left : (unsigned)b.ty;
        const unsigned kk = rem / tyh;
        ijk[1] = b.lo[1] + (int)(yt * (unsigned)b.ty + (rem - kk * tyh));
        ijk[2] = b.lo[2] + (int)kk;
    } else {
        ijk[1] = b.lo[1] + (int)(row % (unsigned)b.ny);
        ijk[2] = b.lo[2] + (int)(row / (unsigned)b.ny);
    }
    const bool owner = live && lane < 63;
    const bool f0 = ijk[0] <= b.hi0 + 1, f1 = ijk[0] + 1 <= b.hi0 + 1;          // faces of nodal(bx, x)
    const bool zA = owner && ijk[0] <= b.hi0, zB = owner && ijk[0] + 1 <= b.hi0; // zones of bx
    const unsigned c = goff(t, ijk[0], ijk[1], ijk[2]);

    double R[2][NFIN];
    final_body<0, false, LIM, false, GEN>(t, ijk, owner && f0, owner && f1, c, Q, S, g, U, fluxes, mass, qe, hdtdy, hdtdz, dt,
                                     area0, g.dx[0], acc_hi, assign, P, R);
    double Rn[NFIN];                                   // face i+2
#pragma unroll
    for (int m = 0; m < NFIN; ++m) Rn[m] = __shfl_down(R[0][m], 1, 64);

    // Castro::consup_hydro (Castro_ctu.cpp:11-86) for the zones i and i+1
    double dtmin = 1.e200, rmin_raw = 1.e300, dtmin1 = 1.e200;
    if (zA) {
        const Str s = gstr(t);
        const unsigned sy = s.y, sz = s.z;
        const long NC = t.NC;
        const double volinv = 1.0 / vol;
        const double* F1 = S.FL[1];
        const double* F2 = S.FL[2];
        const unsigned cn = foff(Unew, ijk[0], ijk[1], ijk[2]);
        const unsigned ci = foff(U, ijk[0], ijk[1], ijk[2]);
        // gamma_law_edges: the species record of FL[y], FL[z] is their mass record (not stored)
        constexpr int rec[NUM_STATE] = { GRHO, GMX, GMY, GMZ, GE, GEI, -1, (gamma_law_edges(GEN) && !LIM) ? GRHO : GX };
        double un[2][NUM_STATE];
        // one species, gamma-law gas, clean_state fused in (gamma_law_edges): the temperature and the species of the old state are
        // dead -- computeTemp overwrites the one, normalize_species makes rho X = rho of the other -- and are not read
        constexpr bool DEAD_TX = gamma_law_edges(GEN) && !LIM && CLEAN;
        // The evolved (rho e).  With clean_state fused in it is wanted only where reset_internal_energy keeps it (clean_zone: cold
        // hypersonic gas, e/E <= eta2); everywhere else clean_zone overwrites it unseen.  So its operands that nothing else reads
        // -- the old UEINT, the GEI records of FL[y], FL[z] and their eight GPG / GUG values -- are loaded zone by zone (`load_e`)
        // and combined (`eint_new`: the expression and order of consup_hydro below, the x faces from R / Rn) when clean_zone asks
        // for the value.  Switched off (lazy_eint_on): loaded for every zone as before.  The arithmetic has one site per zone of the pair
        // either way, so the switch cannot change a bit.
        double eu0, ey0, ey1, ez0, ez1, py0, py1, uy0, uy1, pz0, pz1, uz0, uz1;
        auto load_e = [&](int w) {
            const unsigned o = 8u * (unsigned)w;
            eu0 = from_sborder ? ldg(U.p + UEINT * U.sn, ci + o) : ldg(Unew.p + UEINT * Unew.sn, cn + o);
            ey0 = ldg(F1 + (long)GEI * NC, c + o); ey1 = ldg(F1 + (long)GEI * NC, c + sy + o);
            ez0 = ldg(F2 + (long)GEI * NC, c + o); ez1 = ldg(F2 + (long)GEI * NC, c + sz + o);
            py0 = ldg(F1 + GPG * NC, c + o); py1 = ldg(F1 + GPG * NC, c + sy + o);
            uy0 = ldg(F1 + GUG * NC, c + o); uy1 = ldg(F1 + GUG * NC, c + sy + o);
            pz0 = ldg(F2 + GPG * NC, c + o); pz1 = ldg(F2 + GPG * NC, c + sz + o);
            uz0 = ldg(F2 + GUG * NC, c + o); uz1 = ldg(F2 + GUG * NC, c + sz + o);
        };
        auto eint_new = [&](int w) -> double {
            const double* Rl = w ? R[1] : R[0];       // low and high x face of zone w
            const double* Rh = w ? Rn : R[1];
            double e = eu0 + dt * (Rl[GEI] * area0 - Rh[GEI] * area0 + ey0 * area1 - ey1 * area1 + ez0 * area2 - ez1 * area2) * volinv;
            double pdu = (Rh[GPG] + Rl[GPG]) * (Rh[GUG] * area0 - Rl[GUG] * area0);
            pdu += (py1 + py0) * (uy1 * area1 - uy0 * area1);
            pdu += (pz1 + pz0) * (uz1 * area2 - uz0 * area2);
            pdu = 0.5 * pdu * volinv;
            return e - dt * pdu;
        };
#pragma unroll
        for (int m = 0; m < NUM_STATE; ++m) {
            if (DEAD_TX && m == UTEMP) { un[0][m] = un[1][m] = 0.0; continue; }
            if (DEAD_TX && m == UFS) { un[0][m] = un[0][URHO]; un[1][m] = un[1][URHO]; continue; }
            if (CLEAN && m == UEINT) { un[0][m] = un[1][m] = 0.0; continue; }     // clean_zone asks for it, or overwrites it
            const D2 u0 = from_sborder ? ldg2(U.p + m * U.sn, ci) : ldg2(Unew.p + m * Unew.sn, cn);
            if (m == UTEMP) { un[0][m] = u0.a; un[1][m] = u0.b; continue; }       // zero flux
            const int r = rec[m];
            const D2 y0 = ldg2(F1 + (long)r * NC, c), y1 = ldg2(F1 + (long)r * NC, c + sy);
            const D2 z0 = ldg2(F2 + (long)r * NC, c), z1 = ldg2(F2 + (long)r * NC, c + sz);
            un[0][m] = u0.a + dt * (R[0][r] * area0 - R[1][r] * area0 + y0.a * area1 - y1.a * area1 + z0.a * area2 - z1.a * area2) * volinv;
            un[1][m] = u0.b + dt * (R[1][r] * area0 - Rn[r] * area0 + y0.b * area1 - y1.b * area1 + z0.b * area2 - z1.b * area2) * volinv;
            if (m == UEINT) {
                const D2 py0 = ldg2(F1 + GPG * NC, c), py1 = ldg2(F1 + GPG * NC, c + sy);
                const D2 uy0 = ldg2(F1 + GUG * NC, c), uy1 = ldg2(F1 + GUG * NC, c + sy);
                const D2 pz0 = ldg2(F2 + GPG * NC, c), pz1 = ldg2(F2 + GPG * NC, c + sz);
                const D2 uz0 = ldg2(F2 + GUG * NC, c), uz1 = ldg2(F2 + GUG * NC, c + sz);
                double pdu = (R[1][GPG] + R[0][GPG]) * (R[1][GUG] * area0 - R[0][GUG] * area0);
                pdu += (py1.a + py0.a) * (uy1.a * area1 - uy0.a * area1);
                pdu += (pz1.a + pz0.a) * (uz1.a * area2 - uz0.a * area2);
                pdu = 0.5 * pdu * volinv;
                un[0][m] = un[0][m] - dt * pdu;
                pdu = (Rn[GPG] + R[1][GPG]) * (Rn[GUG] * area0 - R[1][GUG] * area0);
                pdu += (py1.b + py0.b) * (uy1.b * area1 - uy0.b * area1);
                pdu += (pz1.b + pz0.b) * (uz1.b * area2 - uz0.b * area2);
                pdu = 0.5 * pdu * volinv;
                un[1][m] = un[1][m] - dt * pdu;
            }
        }
        if (CLEAN) {
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                if (w == 1 && !zB) continue;
                rmin_raw = fmin(rmin_raw, nan_guard(un[w][URHO]));
                double d1, d2;
                bool e_loaded = false;
                if (!lazy_eint_on(assign)) { load_e(w); e_loaded = true; }
                clean_zone_dt(P, ntimes, g.dx[0], g.dx[1], g.dx[2], un[w][URHO], un[w][UMX], un[w][UMY], un[w][UMZ], un[w][UEDEN], un[w][UEINT], un[w][UTEMP], un[w][UFS], d1, d2,
                              [&]() { if (!e_loaded) load_e(w); return eint_new(w); }, false);
                dtmin1 = fmin(dtmin1, d1);
                dtmin = fmin(dtmin, d2);
            }
        }
#pragma unroll
        for (int m = 0; m < NUM_STATE; ++m) {
            if (m == UTEMP && !CLEAN && !from_sborder) continue;     // unchanged in place
            if (zB) stg2(Unew.p + m * Unew.sn, cn, un[0][m], un[1][m]);
            else stg(Unew.p + m * Unew.sn, cn, un[0][m]);
        }
    }
    if (CLEAN && red) wave_min3_atomic(dtmin, rmin_raw, dtmin1, red);     // per wave: no barrier, any workgroup size
}

// ---------------------------------------------------------------------------------------
// k_final_tile (round 5): the WHOLE final stage in one zone-centred launch -- trans_final, the final Riemann solves and the
// flux tail (apply_av, species flux, scaling, fluxes / mass_fluxes / qe) for x, y and z, consup_hydro and the fused
// clean_state / CFL reduction -- so that no final flux ever goes through HBM on its way to the update: FL[y], FL[z] (16 planes
// written, 16 read), two of the three reads of Sborder, div(u) and the sound speed (14 planes) leave the step, 48 of 291 passes.
//   A workgroup owns RY x RZ rows of zones of one run of 63 x-slots, a wave per row (wave loads stay 1-KB pieces of one row).
//   Every wave solves the low y-face and the low z-face of its row; a zone's HIGH y / z fluxes are the low ones of the rows above:
//   handed over through LDS (8-value records: six fluxes, Godunov u_n and p), the faces on top of the tile (RY + RZ face rows) are
//   dealt to the waves and solved a second time (they belong to the tiles above; only the box's last faces are stored from here).
//   One barrier; then the x faces (the high one from the next lane, as in k_finalx_consup) and the update.  Own low z
//   contribution rides in registers (16 doubles), own low y records in LDS: 18 rows x 8 KB = 144 KB, one workgroup of 8 waves per CU.
//   `contract` build, default solver set, no flux limiters.  Sum order of consup_hydro as in the reference (Castro_ctu.cpp:40-70).
// ---------------------------------------------------------------------------------------
struct FinalOut { DFab fl[3], mass[3], qe[3]; int acc_hi[3]; };
constexpr int NRF = 8;                             // handed-over record: GRHO GMX GMY GMZ GE GEI, then GUG, GPG

__device__ __forceinline__ void frec_put(double* __restrict__ L, int row, int w, int lane, const double R[NFIN])
{
    double* p = L + ((row * 2 + w) * NRF) * 64 + lane;
#pragma unroll
    for (int n = 0; n < 6; ++n) p[n * 64] = R[n];
    p[6 * 64] = R[GUG]; p[7 * 64] = R[GPG];
}
__device__ __forceinline__ void frec_get(const double* __restrict__ L, int row, int w, int lane, double R[NRF])
{
    const double* p = L + ((row * 2 + w) * NRF) * 64 + lane;
#pragma unroll
    for (int n = 0; n < NRF; ++n) R[n] = p[n * 64];
}

#ifdef CAD_NUMERICS_CONTRACT
template <bool CLEAN, int GEN, int RY, int RZ>
__global__ void __launch_bounds__(64 * RY * RZ)
k_final_tile(Tile t, TileRows b, const double* __restrict__ Q, DevScratch S, DevGeom g, DFab U, FinalOut O, DFab Unew,
             double dt, double area0, double area1, double area2, double vol, int assign, int from_sborder, DevParams P,
             int ntimes, double* red)
{
    static_assert(gamma_law_edges(GEN), "k_final_tile: gamma_law_edges instantiations only");
    static_assert(GRHO == 0 && GEI == 5, "record order");
    RETURN_IF_BATCH_FAILED();
    if (P.dtp) dt = P.dtp[6];
    const double hdtdx = 0.5 * dt / g.dx[0], hdtdy = 0.5 * dt / g.dx[1], hdtdz = 0.5 * dt / g.dx[2];
    constexpr int ROWD = 2 * NRF * 64;              // doubles per face row
    __shared__ double rec[((RY + 1) * RZ + RY * RZ) * ROWD];
    double* const Ly = rec;                         // y records of face rows a = 0 .. RY of every kr: row kr (RY + 1) + a
    double* const Lz = rec + (RY + 1) * RZ * ROWD;  // z records of face rows b = 1 .. RZ of every jr: row (b - 1) RY + jr

    unsigned bid = blockIdx.x;
    bid = (bid & 7u) * (b.nb >> 3) + (bid >> 3);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int jr = wave % RY, kr = wave / RY;
    const unsigned total = (unsigned)b.nslot * (unsigned)b.ntj * (unsigned)b.ntk;
    unsigned pos = bid * 63u + (unsigned)lane;
    const bool live = pos < total;
    if (!live) pos = total - 1u;
    const bool owner = live && lane < 63;            // lane 63 repeats the first slot of the next run: it only hands its x record over
    const unsigned tile = pos / (unsigned)b.nslot;
    const int xs = (int)(pos - tile * (unsigned)b.nslot);
    const unsigned per_band = (unsigned)b.band * (unsigned)b.ntk;
    const unsigned bd = tile / per_band;
    const unsigned rem = tile - bd * per_band;
    const unsigned left = (unsigned)b.ntj - bd * (unsigned)b.band;
    const unsigned bw = left < (unsigned)b.band ? left : (unsigned)b.band;
    const unsigned tk = rem / bw;
    const unsigned tj = bd * (unsigned)b.band + (rem - tk * bw);
    const int j0 = b.lo[1] + (int)tj * RY, k0 = b.lo[2] + (int)tk * RZ;
    const int hj = b.lo[1] + b.ny - 1, hk = b.lo[2] + b.nz - 1;            // last rows of zones
    const int i = b.lo[0] + 2 * xs;
    const int j = j0 + jr, k = k0 + kr;
    const bool zrow = j <= hj && k <= hk;
    const bool f0 = i <= b.hi0 + 1, f1 = i + 1 <= b.hi0 + 1;               // faces of nodal(bx, x)
    const bool iA = i <= b.hi0, iB = i + 1 <= b.hi0;                      // zones of bx
    const bool zA = owner && zrow && iA, zB = owner && zrow && iB;
    const Str s = gstr(t);
    const long NC = t.NC;

    // ---- own low z-faces (face row k of the zones (j, k)): flux arrays, the record for the row below, the own contribution
    double accz[2][6], pz[2], uz[2];
    {
        const bool ok = owner && j <= hj && k <= hk + 1;
        int ijk[3] = { i, j <= hj ? j : hj, k <= hk + 1 ? k : hk + 1 };
        double R[2][NFIN];
        final_body<2, false, false, false, GEN>(t, ijk, ok && iA, ok && iB, goff(t, ijk[0], ijk[1], ijk[2]), Q, S, g, U, O.fl[2], O.mass[2], O.qe[2],
                                                hdtdx, hdtdy, dt, area2, g.dx[2], O.acc_hi[2], assign, P, R);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
            for (int m = 0; m < 6; ++m) accz[w][m] = R[w][m];
            pz[w] = R[w][GPG]; uz[w] = R[w][GUG];
            if (kr >= 1) frec_put(Lz, (kr - 1) * RY + jr, w, lane, R[w]);
        }
    }
    // ---- own low y-faces
    {
        const bool ok = owner && j <= hj + 1 && k <= hk;
        int ijk[3] = { i, j <= hj + 1 ? j : hj + 1, k <= hk ? k : hk };
        double R[2][NFIN];
        final_body<1, false, false, false, GEN>(t, ijk, ok && iA, ok && iB, goff(t, ijk[0], ijk[1], ijk[2]), Q, S, g, U, O.fl[1], O.mass[1], O.qe[1],
                                                hdtdx, hdtdz, dt, area1, g.dx[1], O.acc_hi[1], assign, P, R);
        frec_put(Ly, kr * (RY + 1) + jr, 0, lane, R[0]);
        frec_put(Ly, kr * (RY + 1) + jr, 1, lane, R[1]);
    }
    // ---- the face rows on top of the tile: they are the low faces of the tiles above (solved there too); stored from here only
    //      where they are the last faces of the box
    if (wave < RZ) {
        const int jf = j0 + RY, kf = k0 + wave;
        const bool ok = owner && jf == hj + 1 && kf <= hk;
        int ijk[3] = { i, jf <= hj + 1 ? jf : hj + 1, kf <= hk ? kf : hk };
        double R[2][NFIN];
        final_body<1, false, false, false, GEN>(t, ijk, ok && iA, ok && iB, goff(t, ijk[0], ijk[1], ijk[2]), Q, S, g, U, O.fl[1], O.mass[1], O.qe[1],
                                                hdtdx, hdtdz, dt, area1, g.dx[1], O.acc_hi[1], assign, P, R);
        frec_put(Ly, wave * (RY + 1) + RY, 0, lane, R[0]);
        frec_put(Ly, wave * (RY + 1) + RY, 1, lane, R[1]);
    } else if (wave < RZ + RY) {
        const int jf = j0 + (wave - RZ), kf = k0 + RZ;
        const bool ok = owner && kf == hk + 1 && jf <= hj;
        int ijk[3] = { i, jf <= hj ? jf : hj, kf <= hk + 1 ? kf : hk + 1 };
        double R[2][NFIN];
        final_body<2, false, false, false, GEN>(t, ijk, ok && iA, ok && iB, goff(t, ijk[0], ijk[1], ijk[2]), Q, S, g, U, O.fl[2], O.mass[2], O.qe[2],
                                                hdtdx, hdtdy, dt, area2, g.dx[2], O.acc_hi[2], assign, P, R);
        frec_put(Lz, (RZ - 1) * RY + (wave - RZ), 0, lane, R[0]);
        frec_put(Lz, (RZ - 1) * RY + (wave - RZ), 1, lane, R[1]);
    }
    __syncthreads();

    // ---- the x faces of the row and Castro::consup_hydro (Castro_ctu.cpp:11-86) for the zones i and i+1
    int ijk[3] = { i, j <= hj ? j : hj, k <= hk ? k : hk };
    const unsigned c = goff(t, ijk[0], ijk[1], ijk[2]);
    double R[2][NFIN];
    final_body<0, false, false, false, GEN>(t, ijk, owner && zrow && f0, owner && zrow && f1, c, Q, S, g, U, O.fl[0], O.mass[0], O.qe[0],
                                            hdtdy, hdtdz, dt, area0, g.dx[0], O.acc_hi[0], assign, P, R);
    double Rn[NFIN];                                   // face i+2
#pragma unroll
    for (int m = 0; m < NFIN; ++m) Rn[m] = __shfl_down(R[0][m], 1, 64);

    double dtmin = 1.e200, rmin_raw = 1.e300, dtmin1 = 1.e200;
    if (zA) {
        const double volinv = 1.0 / vol;
        const unsigned cn = foff(Unew, ijk[0], ijk[1], ijk[2]);
        const unsigned ci = foff(U, ijk[0], ijk[1], ijk[2]);
        double y0[2][NRF], y1[2][NRF], z1[2][NRF];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            frec_get(Ly, kr * (RY + 1) + jr, w, lane, y0[w]);
            frec_get(Ly, kr * (RY + 1) + jr + 1, w, lane, y1[w]);
            frec_get(Lz, kr * RY + jr, w, lane, z1[w]);
        }
        constexpr int rec_of[NUM_STATE] = { GRHO, GMX, GMY, GMZ, GE, GEI, -1, GRHO };       // the species flux is the mass flux
        constexpr bool DEAD_TX = CLEAN;              // the temperature and the species of the old state are dead (see k_finalx_consup)
        double un[2][NUM_STATE];
#pragma unroll
        for (int m = 0; m < NUM_STATE; ++m) {
            if (DEAD_TX && m == UTEMP) { un[0][m] = un[1][m] = 0.0; continue; }
            if (DEAD_TX && m == UFS) { un[0][m] = un[0][URHO]; un[1][m] = un[1][URHO]; continue; }
            const D2 u0 = from_sborder ? ldg2(U.p + m * U.sn, ci) : ldg2(Unew.p + m * Unew.sn, cn);
            if (m == UTEMP) { un[0][m] = u0.a; un[1][m] = u0.b; continue; }       // zero flux
            const int r = rec_of[m];
            un[0][m] = u0.a + dt * (R[0][r] * area0 - R[1][r] * area0 + y0[0][r] * area1 - y1[0][r] * area1 + accz[0][r] * area2 - z1[0][r] * area2) * volinv;
            un[1][m] = u0.b + dt * (R[1][r] * area0 - Rn[r] * area0 + y0[1][r] * area1 - y1[1][r] * area1 + accz[1][r] * area2 - z1[1][r] * area2) * volinv;
            if (m == UEINT) {
                double pdu = (R[1][GPG] + R[0][GPG]) * (R[1][GUG] * area0 - R[0][GUG] * area0);
                pdu += (y1[0][7] + y0[0][7]) * (y1[0][6] * area1 - y0[0][6] * area1);
                pdu += (z1[0][7] + pz[0]) * (z1[0][6] * area2 - uz[0] * area2);
                pdu = 0.5 * pdu * volinv;
                un[0][m] = un[0][m] - dt * pdu;
                pdu = (Rn[GPG] + R[1][GPG]) * (Rn[GUG] * area0 - R[1][GUG] * area0);
                pdu += (y1[1][7] + y0[1][7]) * (y1[1][6] * area1 - y0[1][6] * area1);
                pdu += (z1[1][7] + pz[1]) * (z1[1][6] * area2 - uz[1] * area2);
                pdu = 0.5 * pdu * volinv;
                un[1][m] = un[1][m] - dt * pdu;
            }
        }
        if (CLEAN) {
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                if (w == 1 && !zB) continue;
                rmin_raw = fmin(rmin_raw, nan_guard(un[w][URHO]));
                double d1, d2;
                clean_zone_dt(P, ntimes, g.dx[0], g.dx[1], g.dx[2], un[w][URHO], un[w][UMX], un[w][UMY], un[w][UMZ], un[w][UEDEN], un[w][UEINT], un[w][UTEMP], un[w][UFS], d1, d2);
                dtmin1 = fmin(dtmin1, d1);
                dtmin = fmin(dtmin, d2);
            }
        }
#pragma unroll
        for (int m = 0; m < NUM_STATE; ++m) {
            if (m == UTEMP && !CLEAN && !from_sborder) continue;     // unchanged in place
            if (zB) stg2(Unew.p + m * Unew.sn, cn, un[0][m], un[1][m]);
            else stg(Unew.p + m * Unew.sn, cn, un[0][m]);
        }
    }
    if (CLEAN && red) wave_min3_atomic(dtmin, rmin_raw, dtmin1, red);
}
#endif

// ---------------------------------------------------------------------------------------
// host-side launcher
// ---------------------------------------------------------------------------------------
// the one table of the launcher's environment variables (defaults: LaunchKnobs, ctu_kernels.h)
LaunchKnobs launch_knobs_from_env()
{
    auto knob = [](const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; };
    auto wg_knob = [&](const char* name, int dflt) { const int v = knob(name, dflt); return (v == 64 || v == 128 || v == 256) ? v : dflt; };
    const LaunchKnobs d;
    LaunchKnobs K;
    K.tile_rows = knob("CASTRO_AMD_TILE_ROWS", d.tile_rows);
    K.trace_tile_rows = knob("CASTRO_AMD_TRACE_TILE_ROWS", d.trace_tile_rows);
    K.fold_tile_rows = knob("CASTRO_AMD_FOLD_TILE_ROWS", d.fold_tile_rows);
    K.fused_tile_rows = knob("CASTRO_AMD_FUSED_TILE_ROWS", d.fused_tile_rows);
    K.wg = wg_knob("CASTRO_AMD_WG", d.wg);
    K.final_wg = wg_knob("CASTRO_AMD_FINAL_WG", d.final_wg);
    K.fused_wg = wg_knob("CASTRO_AMD_FUSED_WG", d.fused_wg);
    K.xpad = knob("CASTRO_AMD_XPAD", d.xpad);
    K.fuse_consup = knob("CASTRO_AMD_FUSE_CONSUP", d.fuse_consup);
    K.fold_r1 = knob("CASTRO_AMD_FOLD_R1", d.fold_r1);
    K.fold_tile = knob("CASTRO_AMD_FOLD_TILE", d.fold_tile);
    K.final_tile = knob("CASTRO_AMD_FINAL_TILE", d.final_tile);
    K.gl_sources = knob("CASTRO_AMD_GL_SOURCES", d.gl_sources);
    K.gl_plm = knob("CASTRO_AMD_GL_PLM", d.gl_plm);
    K.divu_in_trace = knob("CASTRO_AMD_DIVU_IN_TRACE", d.divu_in_trace);
    K.trace_one_zone = knob("CASTRO_AMD_TRACE_ONE_ZONE", d.trace_one_zone);
    K.side_stream = knob("CASTRO_AMD_SIDE_STREAM", d.side_stream);
    K.lazy_loads = knob("CASTRO_AMD_LAZY_LOADS", d.lazy_loads);
    return K;
}

// Workgroup order and size of a launch: rows per y-tile (0: plain row-major order) and threads per workgroup.  The knobs whose
// -1 / 0 stands for "the general value" are resolved here and nowhere else.
struct Shape { int ty; unsigned wg; };
static Shape plain_shape(const LaunchKnobs& K) { return { K.tile_rows, (unsigned)K.wg }; }
static Shape trace_shape(const LaunchKnobs& K) { return { K.trace_tile_rows >= 0 ? K.trace_tile_rows : K.tile_rows, (unsigned)K.wg }; }
static Shape fold_shape(const LaunchKnobs& K) { return { K.fold_tile_rows >= 0 ? K.fold_tile_rows : K.tile_rows, (unsigned)K.wg }; }
static Shape final_shape(const LaunchKnobs& K) { return { K.tile_rows, (unsigned)(K.final_wg > 0 ? K.final_wg : K.wg) }; }   // k_final<y>, k_final<z>

static LinBox linbox(const int lo[3], const int hi[3], Shape sh, long& n)
{
    LinBox b;
    n = 1;
    for (int d = 0; d < 3; ++d) { b.lo[d] = lo[d]; b.n[d] = hi[d] - lo[d] + 1; n *= b.n[d]; }
    b.ty = sh.ty;
    b.w = 1;
    b.hi0 = hi[0];
    b.wg = sh.wg;
    b.nb = (unsigned)((n + b.wg - 1) / b.wg);
    if (b.ty > 0) b.nb = (b.nb + 7u) & ~7u;
    return b;
}

// pairs of x-adjacent zones: thread ii of a row handles lo[0] + 2 ii and, if <= hi0, the next one
static LinBox linbox2(const int lo[3], const int hi[3], Shape sh, long& n)
{
    LinBox b = linbox(lo, hi, sh, n);
    b.w = 2;
    b.n[0] = (b.n[0] + 1) / 2;
    n = (long)b.n[0] * b.n[1] * b.n[2];
    b.nb = (unsigned)((n + b.wg - 1) / b.wg);
    if (b.ty > 0) b.nb = (b.nb + 7u) & ~7u;
    return b;
}

// ---- launch geometry shared by launch_ctu_hydro and launch_ctu_hydro_level (which must give every box what the former gives it)
static SkipBox grow(const Tile& t, int n)
{
    SkipBox b;
    for (int d = 0; d < 3; ++d) { b.lo[d] = t.lo[d] - n; b.hi[d] = t.hi[d] + n; }
    return b;
}
// the faces of direction d of bx, grown by n in the transverse directions
static SkipBox face_box(const Tile& t, int d, int n)
{
    SkipBox b = grow(t, n);
    b.lo[d] = t.lo[d]; b.hi[d] = t.hi[d] + 1;
    return b;
}
// the kernels whose waves overlap by one slot (fold_thread) take 63 new slots per wave
static long slot_waves(long slots) { return (slots + 62) / 63; }
// x slots of a row of the final stage: pairs of x faces of bx
static int face_slots(const Tile& t) { const int nx = t.hi[0] - t.lo[0] + 1; return (nx + 1) / 2 + 1; }
// workgroups of k_trans1_fold_lds over the pairs of b
static unsigned fold_blocks(const LinBox& b)
{
    const long n = (long)b.n[0] * b.n[1] * b.n[2];
    unsigned nb = (unsigned)((slot_waves(n) + FOLD_WG / 64 - 1) / (FOLD_WG / 64));
    if (b.ty > 0) nb = (nb + 7u) & ~7u;
    return nb;
}
// k_finalx_consup over bx
static XRows x_rows(const Tile& t, const LaunchKnobs& K)
{
    XRows xr;
    for (int d = 0; d < 3; ++d) xr.lo[d] = t.lo[d];
    xr.hi0 = t.hi[0];
    xr.nslot = face_slots(t); xr.ny = t.hi[1] - t.lo[1] + 1; xr.nz = t.hi[2] - t.lo[2] + 1;
    xr.ty = K.fused_tile_rows;
    xr.wv = (unsigned)K.fused_wg / 64u;
    xr.nb = ((unsigned)((slot_waves((long)xr.nslot * xr.ny * xr.nz) + xr.wv - 1) / xr.wv) + 7u) & ~7u;
    return xr;
}
// an ry x rz tile of rows per workgroup (k_trans1_tile, k_final_tile): nslot x ny x nz slots from lo on, bands of band_rows rows (0: one band)
static TileRows tile_rows(const int lo[3], int hi0, int nslot, int ny, int nz, int ry, int rz, int band_rows)
{
    TileRows tr;
    for (int d = 0; d < 3; ++d) tr.lo[d] = lo[d];
    tr.hi0 = hi0;
    tr.nslot = nslot; tr.ny = ny; tr.nz = nz;
    tr.ntj = (ny + ry - 1) / ry; tr.ntk = (nz + rz - 1) / rz;
    tr.band = band_rows > 0 ? (band_rows + ry - 1) / ry : tr.ntj;
    tr.nb = ((unsigned)slot_waves((long)tr.nslot * tr.ntj * tr.ntk) + 7u) & ~7u;
    return tr;
}
// cdtdx = dt/dx/3 (Castro_ctu_hydro.cpp:688-690); hdtdx = 0.5*dt/dx (:684-686)
struct StepConsts { double cdtdx, cdtdy, cdtdz, hdtdx, hdtdy, hdtdz, area0, area1, area2, vol; };
static StepConsts step_consts(const DevGeom& g, double dt)
{
    return { dt / g.dx[0] / 3.0, dt / g.dx[1] / 3.0, dt / g.dx[2] / 3.0, 0.5 * dt / g.dx[0], 0.5 * dt / g.dx[1], 0.5 * dt / g.dx[2],
             g.dx[1] * g.dx[2], g.dx[0] * g.dx[2], g.dx[0] * g.dx[1], g.dx[0] * g.dx[1] * g.dx[2] };
}

// one launch of `kern` over [lo, hi] on `strm` in the shape `sh`: BOX = linbox (a zone per thread) or linbox2 (an x pair per thread)
#define KL_ON(strm, BOX, name, kern, sh, lo, hi, ...)                                        \
    do {                                                                                     \
        long n_;                                                                             \
        LinBox b_ = BOX(lo, hi, sh, n_);                                                     \
        if (n_ > 0) {                                                                        \
            prof_begin(prof, name, strm);                                                    \
            hipLaunchKernelGGL(kern, dim3(b_.nb), dim3(b_.wg), 0, strm, t, b_, __VA_ARGS__); \
            prof_end(prof, strm);                                                            \
        }                                                                                    \
    } while (0)
#define KL(name, kern, sh, lo, hi, ...) KL_ON(stream, linbox, name, kern, sh, lo, hi, __VA_ARGS__)
#define KL2(name, kern, sh, lo, hi, ...) KL_ON(stream, linbox2, name, kern, sh, lo, hi, __VA_ARGS__)

#define K_R1_0(V) (k_riemann1<0, false, V>)
#define K_R1_1(V) (k_riemann1<1, false, V>)
#define K_R1_2(V) (k_riemann1<2, false, V>)
#define K_T1(V) (k_trans1<false, 7, V>)
#define K_FY(V) (k_final<1, false, false, V>)
#define K_FZ(V) (k_final<2, false, false, V>)
// the instantiation of a kernel template for `solv` (see interface_flux): KERN(2), KERN(1) or KERN(0)
#define KL2_SOLV(name, KERN, sh, lo, hi, ...)                                                \
    do {                                                                                     \
        if (solv == 2) KL2(name, KERN(2), sh, lo, hi, __VA_ARGS__);                          \
        else if (solv == 1) KL2(name, KERN(1), sh, lo, hi, __VA_ARGS__);                     \
        else KL2(name, KERN(0), sh, lo, hi, __VA_ARGS__);                                    \
    } while (0)

// outer box minus inner box as up to six slabs: z slabs over the full x,y extent, y slabs over the inner z range,
// x slabs over the inner y,z range (thin in x: a wavefront then covers many rows, no idle lanes)
static int shell_boxes(const int olo[3], const int ohi[3], const int ilo[3], const int ihi[3], int lo[6][3], int hi[6][3])
{
    int n = 0;
    auto add = [&](int x0, int x1, int y0, int y1, int z0, int z1) {
        if (x0 > x1 || y0 > y1 || z0 > z1) return;
        lo[n][0] = x0; hi[n][0] = x1; lo[n][1] = y0; hi[n][1] = y1; lo[n][2] = z0; hi[n][2] = z1; ++n;
    };
    add(olo[0], ohi[0], olo[1], ohi[1], olo[2], ilo[2] - 1);
    add(olo[0], ohi[0], olo[1], ohi[1], ihi[2] + 1, ohi[2]);
    add(olo[0], ohi[0], olo[1], ilo[1] - 1, ilo[2], ihi[2]);
    add(olo[0], ohi[0], ihi[1] + 1, ohi[1], ilo[2], ihi[2]);
    add(olo[0], ilo[0] - 1, ilo[1], ihi[1], ilo[2], ihi[2]);
    add(ihi[0] + 1, ohi[0], ilo[1], ihi[1], ilo[2], ihi[2]);
    return n;
}

int launch_ctu_hydro(const Tile& t, const DevScratch& S, const DFab& Sborder, const DFab& Src, const DFab& Snew,
                     const DFab fluxes[3], const DFab mass[3], const DFab qe[3],
                     const DevGeom& g, const DevParams& P, double dt, int flags, const int acc_hi[3],
                     int* d_status, hipStream_t stream, Profiler* prof, int clean_ntimes, double* red, const DFab& SrcCorr,
                     const LaunchAux& aux)
{
    const LevelTab nolv = { nullptr, nullptr, 0 };       // one box: the kernels take their arguments as passed
    const LaunchKnobs& K = aux.knobs;
    const Shape plain = plain_shape(K);
    // Staged execution (CASTRO_AMD_STAGE_A / _B): A = what needs no ghost zone of Sborder -- ctoprim on the valid
    // zones, PPM tracing on grow(bx, -3) -- so that a caller can run it while the halo exchange is in flight;
    // B = the rest (ctoprim on the ghost shell, tracing on the remaining zones, everything downstream).
    // Only the no-source PPM path is split; otherwise A is empty and B is the whole update.
    // ppm_temp_fix = 2: the first solves go through k_riemann1<D, TFIX>: no fused x solve, no staging
    const bool tfix = P.ppm_temp_fix == 2 && P.riemann_solver != 2;
    // hybrid_riemann = 1: the fused x solve of stage A would read the shock flags, which k_divu writes in stage B
    const bool splittable = !Src.p && P.ppm_type == 1 && !tfix && P.hybrid_riemann != 1;
    // which solvers the kernels of the default-option path contain (interface_flux<D, SOLV>): 0 default only, 1 all but CG, 2 all
    // GEN == 0 instantiations keep their transverse-stage records in the 7-plane state form (store_f1: QI), so they are
    // used only where EVERY kernel of the call is one: the all-default path.  A non-default final stage, the flux
    // limiters, transverse_reset_rhoe and ppm_temp_fix run kernels of the full solver set (flux-form records).
    const bool plain_path = !(P.ppm_temp_fix == 2 && P.riemann_solver != 2) && P.reset_rhoe != 1 && K.fuse_consup == 1
                            && P.limit_small_dens != 1 && P.limit_large_vel != 1;
    // gamma_law_edges (contract build): the GEN == 0 readers take (rho e) of an edge state from its p, which only the trace
    // kernel of the no-source PPM path promises (k_trace_pair<true, 7, 0>); traces with source terms or PLM run the GEN >= 1 set
    // (round 5: traced source terms keep the identity -- trace_dir<D, SRC, GL> -- so only PLM is left out)
    // (round 6: the PLM trace keeps it too -- trace_plm_dir<D, SRC, GL>.  castro.use_pslope = 1 (the default) gives p a slope of its own:
    // without a source term and away from a Symmetry face it is uslope's expression on half the differences -- the same number in real
    // arithmetic (for the default fourth-order limiter, plm_limiter = 2) --, with one it carries the hydrostatic part and at such a face it
    // drops the differences across it, and the slope of (rho e) would no longer be that of p over (gamma - 1): those runs keep the
    // 7-variable kernels.  CASTRO_AMD_GL_PLM=0 is the A/B knob)
    bool plm_gl = P.ppm_type == 0 && K.gl_plm;
    if (plm_gl && P.use_pslope == 1) {
        if (Src.p) plm_gl = false;
        // pslope is the fourth-order form whatever castro.plm_limiter says: with plm_limiter = 1 the other variables -- (rho e) among
        // them -- take the second-order slope and the two no longer agree (found by the contract test of that option: 1e-2)
        if (P.plm_iorder != 1 && P.plm_limiter != 2) plm_gl = false;
        for (int d = 0; d < 3; ++d) if (g.sym_lo[d] || g.sym_hi[d]) plm_gl = false;
    }
    const bool gl_ok = !gamma_law_edges(0) || ((P.ppm_type == 1 || plm_gl) && (!Src.p || K.gl_sources));
    const int solv = (P.riemann_solver == 1) ? 2 : ((P.riemann_solver == 2 || P.hybrid_riemann == 1 || !plain_path || !gl_ok) ? 1 : 0);
    const int lean_q = (gamma_law_edges(0) && solv == 0) ? (clean_ntimes > 0 ? 3 : 1) : 0;      // see k_ctoprim
    const bool stage_a = (flags & 4) != 0, stage_b = (flags & 8) != 0, staged = stage_a || stage_b;
    const SkipBox none = { { 0, 0, 0 }, { -1, -1, -1 } };
    const SkipBox inner_box = grow(t, -3);
    const bool inner_ok = inner_box.lo[0] <= inner_box.hi[0] && inner_box.lo[1] <= inner_box.hi[1] && inner_box.lo[2] <= inner_box.hi[2];

    // boxes
    const SkipBox ob = grow(t, 1);
    const SkipBox qb = grow(t, 4);      // the zones of Sborder the path reads

    // PPM tracing of the zones of [lo,hi] with the first x Riemann solve fused in, for the faces whose two zones the
    // launch covers; the faces at the workgroup starts follow in a one-thread-per-workgroup launch, those on the
    // x faces of the launch box (lo[0] and hi[0] + 1) are left to the caller.
    // div(u) of the nodes of grow(bx, 1) inside the trace launches (every zone of that box goes through trace_with_xriemann on this
    // path, staged or not) instead of a k_divu_pair launch of its own; the hybrid solver needs k_divu's shock flags before the trace
    const bool divu_in_trace = K.divu_in_trace && !Src.p && P.ppm_type == 1 && !tfix && P.hybrid_riemann != 1 && !K.trace_one_zone;
    auto trace_with_xriemann = [&](const int lo[3], const int hi[3]) {
        // the trace launch and the block-start fix-up share one workgroup order: both get the trace's rows per y-tile
        const Shape trace = trace_shape(K);
#define K_(V) (k_trace_pair<true, 7, V>)
        KL2_SOLV("k_trace", K_, trace, lo, hi, S.Q, S, g, dt, P, none, nolv, divu_in_trace ? 1 : 0);
#undef K_
        long n_;
        LinBox b_ = linbox2(lo, hi, trace, n_);
        if (n_ > 0) {
            prof_begin(prof, "k_riemann1_blockstart", stream);
            auto kbs = solv == 2 ? k_riemann1_blockstart<2> : solv == 1 ? k_riemann1_blockstart<1> : k_riemann1_blockstart<0>;
            hipLaunchKernelGGL(kbs, dim3((b_.nb + 255) / 256), dim3(256), 0, stream, t, b_, S.Q, S, g, P, nolv);
            prof_end(prof, stream);
        }
    };

    if (stage_a) {
        if (splittable) {
            KL("k_ctoprim", k_ctoprim<false>, plain, t.lo, t.hi, Sborder, S.Q, P, d_status, none, 0, nolv, lean_q, 0, ShellBoxes{}, BcKinds{});
            if (inner_ok) trace_with_xriemann(inner_box.lo, inner_box.hi);
        }
        return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
    }
    // The light split (round 6: CASTRO_AMD_STAGE_VALID / _REST): ctoprim -- with the pending clean_states -- on the valid zones
    // is all that runs beside the halo exchange; the ghost shell follows as ONE launch, everything downstream is un-split.
    // CASTRO_AMD_BC_FILL: the zones of grow(bx, 4) outside the problem domain in a non-periodic direction are filled here
    // (k_ctoprim in its boundary-zone mode) from in-domain zones that the launches in front of it have cleaned, instead of by a k_bc_fill before the call.
    const bool light_a = (flags & 16) != 0, light_b = (flags & 32) != 0, fill_bc = (flags & 64) != 0;
    if ((light_a || light_b || fill_bc) && staged) return CASTRO_AMD_ERR_ARG;
    if (light_a && light_b) return CASTRO_AMD_ERR_ARG;
    int ilo[3], ihi[3];                                  // the zones of grow(bx, 4) that hold data when the call starts
    BcKinds M;
    const ShellBoxes no_shell = {};
    bool have_bc = false;
    for (int d = 0; d < 3; ++d) {
        ilo[d] = qb.lo[d]; ihi[d] = qb.hi[d];
        M.lo[d] = g.domlo[d]; M.hi[d] = g.domhi[d];
        M.kind_lo[d] = aux.bc_lo[d] == 0 ? 0 : (aux.bc_lo[d] >= 3 ? 2 : 1);      // Symmetry, SlipWall, NoSlipWall mirror
        M.kind_hi[d] = aux.bc_hi[d] == 0 ? 0 : (aux.bc_hi[d] >= 3 ? 2 : 1);
        if (!fill_bc) continue;
        if (M.kind_lo[d] != 0 && qb.lo[d] < g.domlo[d]) { ilo[d] = g.domlo[d]; have_bc = true; }
        if (M.kind_hi[d] != 0 && qb.hi[d] > g.domhi[d]) { ihi[d] = g.domhi[d]; have_bc = true; }
        // the tile lies inside the domain, and a mirrored ghost layer finds its image among the in-domain zones of this FAB
        if (t.lo[d] < ilo[d] || t.hi[d] > ihi[d]) return CASTRO_AMD_ERR_ARG;
        if (M.kind_lo[d] == 2 && 2 * g.domlo[d] - qb.lo[d] - 1 > ihi[d]) return CASTRO_AMD_ERR_UNSUPPORTED;
        if (M.kind_hi[d] == 2 && 2 * g.domhi[d] - qb.hi[d] + 1 < ilo[d]) return CASTRO_AMD_ERR_UNSUPPORTED;
    }
    auto shell_launch_boxes = [&](const int olo_[3], const int ohi_[3], const int nlo_[3], const int nhi_[3], ShellBoxes& sb) {
        int lo6[6][3], hi6[6][3];
        const int ns = shell_boxes(olo_, ohi_, nlo_, nhi_, lo6, hi6);
        sb.start[0] = 0;
        for (int r = 0; r < 6; ++r) {
            unsigned n = 0;
            if (r < ns) {
                n = 1;
                for (int d = 0; d < 3; ++d) { sb.lo[r][d] = lo6[r][d]; sb.nn[r][d] = hi6[r][d] - lo6[r][d] + 1; n *= (unsigned)sb.nn[r][d]; }
            } else {
                for (int d = 0; d < 3; ++d) { sb.lo[r][d] = 0; sb.nn[r][d] = 1; }
            }
            sb.start[r + 1] = sb.start[r] + n;
        }
        return sb.start[6];
    };
    if (light_a) {
        if (aux.sb_clean > 0) KL("k_ctoprim_clean", k_ctoprim<true>, plain, t.lo, t.hi, Sborder, S.Q, P, d_status, none, aux.sb_clean, nolv, lean_q, 0, no_shell, M);
        else KL("k_ctoprim", k_ctoprim<false>, plain, t.lo, t.hi, Sborder, S.Q, P, d_status, none, 0, nolv, lean_q, 0, no_shell, M);
        return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
    }
    const bool second_half = stage_b && splittable;     // stage A has run on this tile
    int slo[6][3], shi[6][3];
    if (light_b) {
        ShellBoxes sb;
        const unsigned nz_ = shell_launch_boxes(ilo, ihi, t.lo, t.hi, sb);
        if (nz_ > 0) {
            prof_begin(prof, "k_ctoprim_shell", stream);
            LinBox nobox = {};
            if (aux.sb_clean > 0) hipLaunchKernelGGL(k_ctoprim<true>, dim3((nz_ + 255u) / 256u), dim3(256), 0, stream, t, nobox, Sborder, S.Q, P, d_status, none, aux.sb_clean, nolv, lean_q, 1, sb, M);
            else hipLaunchKernelGGL(k_ctoprim<false>, dim3((nz_ + 255u) / 256u), dim3(256), 0, stream, t, nobox, Sborder, S.Q, P, d_status, none, 0, nolv, lean_q, 1, sb, M);
            prof_end(prof, stream);
        }
    } else if (second_half) {
        const int ns = shell_boxes(qb.lo, qb.hi, t.lo, t.hi, slo, shi);
        for (int m = 0; m < ns; ++m) KL("k_ctoprim", k_ctoprim<false>, plain, slo[m], shi[m], Sborder, S.Q, P, d_status, none, 0, nolv, lean_q, 0, no_shell, M);
    } else if (aux.sb_clean > 0) {
        KL("k_ctoprim_clean", k_ctoprim<true>, plain, ilo, ihi, Sborder, S.Q, P, d_status, none, aux.sb_clean, nolv, lean_q, 0, no_shell, M);
    } else {
        KL("k_ctoprim", k_ctoprim<false>, plain, ilo, ihi, Sborder, S.Q, P, d_status, none, 0, nolv, lean_q, 0, no_shell, M);
    }
    if (have_bc) {
        ShellBoxes sb;
        const unsigned nz_ = shell_launch_boxes(qb.lo, qb.hi, ilo, ihi, sb);
        if (nz_ > 0) {
            // the instantiation that did the in-domain zones of this call: one compiled copy of the arithmetic for both
            LinBox nobox = {};
            prof_begin(prof, "k_ctoprim_bc", stream);
            if (aux.sb_clean > 0) hipLaunchKernelGGL(k_ctoprim<true>, dim3((nz_ + 255u) / 256u), dim3(256), 0, stream, t, nobox, Sborder, S.Q, P, d_status, none, 0, nolv, lean_q, 2, sb, M);
            else hipLaunchKernelGGL(k_ctoprim<false>, dim3((nz_ + 255u) / 256u), dim3(256), 0, stream, t, nobox, Sborder, S.Q, P, d_status, none, 0, nolv, lean_q, 2, sb, M);
            prof_end(prof, stream);
        }
    }

    const SkipBox fg[3] = { face_box(t, 0, 1), face_box(t, 1, 1), face_box(t, 2, 1) };     // faces of d, grown by 1 in the transverse dirs
    const SkipBox fb[3] = { face_box(t, 0, 0), face_box(t, 1, 0), face_box(t, 2, 0) };     // faces of d of bx

    // div(u) depends on Q only and is first read by the final stage: on the context's side stream it runs beside the
    // trace kernel (forked from and joined to `stream` by events; the hybrid solver's shock flags are read by the first
    // Riemann solves already, so that form stays in line)
    bool divu_forked = false;
    if (P.hybrid_riemann == 1) { KL("k_divu", k_divu, plain, ob.lo, ob.hi, S.Q, S.DIV, S.SHK, 1.0 / g.dx[0], 1.0 / g.dx[1], 1.0 / g.dx[2]); }
    else if (divu_in_trace) { /* k_trace_pair computes it */ }
    else if (aux.side && K.side_stream) {
        hipEventRecord(aux.ev_fork, stream);
        hipStreamWaitEvent(aux.side, aux.ev_fork, 0);
        KL_ON(aux.side, linbox2, "k_divu", k_divu_pair<false>, plain, ob.lo, ob.hi, S.Q, S.DIV, 1.0 / g.dx[0], 1.0 / g.dx[1], 1.0 / g.dx[2], nolv);
        hipEventRecord(aux.ev_join, aux.side);
        divu_forked = true;
    }
    else { KL2("k_divu", k_divu_pair<false>, plain, ob.lo, ob.hi, S.Q, S.DIV, 1.0 / g.dx[0], 1.0 / g.dx[1], 1.0 / g.dx[2], nolv); }
    // the join must precede the first reader of DIV (and every return path after this point)
    auto join_divu = [&]() { if (divu_forked) { hipStreamWaitEvent(stream, aux.ev_join, 0); divu_forked = false; } };
    bool x_done = false;      // first x Riemann solve already done inside the trace kernel
    bool one_zone_trace = false;
    if (Src.p) {
        const SkipBox q3 = grow(t, 3);
        KL("k_src_to_prim", k_src_to_prim<false>, plain, q3.lo, q3.hi, S.Q, Src, S.SRCQ, P, SrcCorr, dt, lean_q & 1, nolv);
        if (P.ppm_type == 0 && (lean_q & 1)) { KL("k_trace_plm", (k_trace<true, true, gamma_law_edges(0)>), plain, ob.lo, ob.hi, S.Q, S, g, dt, P, nolv); }
        else if (P.ppm_type == 0) { KL("k_trace_plm", (k_trace<true, true>), plain, ob.lo, ob.hi, S.Q, S, g, dt, P, nolv); }
        else if (lean_q & 1) { KL("k_trace", (k_trace<true, false, gamma_law_edges(0)>), plain, ob.lo, ob.hi, S.Q, S, g, dt, P, nolv); }
        else { KL("k_trace", (k_trace<true, false>), plain, ob.lo, ob.hi, S.Q, S, g, dt, P, nolv); }
    } else {
        if (P.ppm_type == 0 && (lean_q & 1)) { KL("k_trace_plm", (k_trace<false, true, gamma_law_edges(0)>), plain, ob.lo, ob.hi, S.Q, S, g, dt, P, nolv); }
        else if (P.ppm_type == 0) { KL("k_trace_plm", (k_trace<false, true>), plain, ob.lo, ob.hi, S.Q, S, g, dt, P, nolv); }
        else if (tfix) { KL2("k_trace", k_trace_pair<false>, plain, ob.lo, ob.hi, S.Q, S, g, dt, P, none, nolv, 0); }
        else if (K.trace_one_zone && !second_half) {
            // A/B (CASTRO_AMD_TRACE_ONE_ZONE=1, round 6): ONE zone per thread at the occupancy that leaves (the kernel of the runs with
            // traced source terms, without the sources), the first x Riemann solve as a launch of its own
            if (lean_q & 1) { KL("k_trace", (k_trace<false, false, gamma_law_edges(0)>), plain, ob.lo, ob.hi, S.Q, S, g, dt, P, nolv); }
            else { KL("k_trace", (k_trace<false, false>), plain, ob.lo, ob.hi, S.Q, S, g, dt, P, nolv); }
            one_zone_trace = true;
        }
        else if (second_half) {
            if (inner_ok) {
                const int ns = shell_boxes(ob.lo, ob.hi, inner_box.lo, inner_box.hi, slo, shi);
                for (int m = 0; m < ns; ++m) trace_with_xriemann(slo[m], shi[m]);
                // the x faces between the inner launch of stage A and the two x slabs
                for (int side = 0; side < 2; ++side) {
                    const int xf = side ? inner_box.hi[0] + 1 : inner_box.lo[0];
                    const int plo[3] = { xf, inner_box.lo[1], inner_box.lo[2] }, phi[3] = { xf, inner_box.hi[1], inner_box.hi[2] };
                    KL2_SOLV("k_riemann1", K_R1_0, plain, plo, phi, S.Q, S, g, P, nolv);
                }
            } else {
                trace_with_xriemann(ob.lo, ob.hi);
            }
        } else {
            trace_with_xriemann(ob.lo, ob.hi);
        }
        x_done = P.ppm_type != 0 && !tfix && !one_zone_trace;
    }
    (void)staged;

    // the first y / z solves folded into the transverse stage (k_trans1_fold): default solver set, default final-stage form
    const bool fold_r1 = K.fold_r1 && solv == 0 && !tfix && P.reset_rhoe != 1 && K.fuse_consup;
    if (tfix) {
        KL2("k_riemann1", (k_riemann1<0, true>), plain, fg[0].lo, fg[0].hi, S.Q, S, g, P, nolv);
        KL2("k_riemann1", (k_riemann1<1, true>), plain, fg[1].lo, fg[1].hi, S.Q, S, g, P, nolv);
        KL2("k_riemann1", (k_riemann1<2, true>), plain, fg[2].lo, fg[2].hi, S.Q, S, g, P, nolv);
    } else {
        if (!x_done) KL2_SOLV("k_riemann1", K_R1_0, plain, fg[0].lo, fg[0].hi, S.Q, S, g, P, nolv);
        if (!fold_r1) {
            KL2_SOLV("k_riemann1", K_R1_1, plain, fg[1].lo, fg[1].hi, S.Q, S, g, P, nolv);
            KL2_SOLV("k_riemann1", K_R1_2, plain, fg[2].lo, fg[2].hi, S.Q, S, g, P, nolv);
        }
    }

    join_divu();
    const auto [cdtdx, cdtdy, cdtdz, hdtdx, hdtdy, hdtdz, area0, area1, area2, vol] = step_consts(g, dt);

    // transverse_reset_rhoe = 1 (non-default) runs its own instantiations: the extra (rho e) flux loads cost the
    // default path 2 % when they sit behind a run-time branch
#define TRANSVERSE_STAGES(RE, LIM)                                                                                \
    do {                                                                                                          \
        KL2("k_trans1", k_trans1<RE>, plain, ob.lo, ob.hi, S.Q, S, g, cdtdx, cdtdy, cdtdz, P);                              \
        KL2("k_final_x", (k_final<0, RE, LIM>), plain, fb[0].lo, fb[0].hi, S.Q, S, g, Sborder, fluxes[0], mass[0], qe[0],      \
            hdtdy, hdtdz, dt, area0, g.dx[0], acc_hi[0], (flags & 2) ? 1 : 0, P, nolv);                                 \
        KL2("k_final_y", (k_final<1, RE, LIM>), plain, fb[1].lo, fb[1].hi, S.Q, S, g, Sborder, fluxes[1], mass[1], qe[1],      \
            hdtdx, hdtdz, dt, area1, g.dx[1], acc_hi[1], (flags & 2) ? 1 : 0, P, nolv);                                 \
        KL2("k_final_z", (k_final<2, RE, LIM>), plain, fb[2].lo, fb[2].hi, S.Q, S, g, Sborder, fluxes[2], mass[2], qe[2],      \
            hdtdx, hdtdy, dt, area2, g.dx[2], acc_hi[2], (flags & 2) ? 1 : 0, P, nolv);                                 \
    } while (0)
    // the flux limiters (non-default too) share one extra pair of instantiations: both flags are tested inside
    const bool lim = P.limit_small_dens == 1 || P.limit_large_vel == 1;
    if (P.reset_rhoe == 1 || tfix) { if (lim) TRANSVERSE_STAGES(true, true); else TRANSVERSE_STAGES(true, false); }
    else if (K.fuse_consup) {
        // y and z first (they write FL[1], FL[2]), then the x faces with the conservative update fused in
        if (fold_r1) {
            long n_;
            LinBox b_ = linbox2(ob.lo, ob.hi, fold_shape(K), n_);
#ifdef CAD_NUMERICS_CONTRACT
            const int fold_tile = K.fold_tile >= 0 ? K.fold_tile : ((b_.n[1] >= 96 && b_.n[2] >= 96 && b_.n[0] >= 48) ? 1 : 0);
            if (n_ > 0 && fold_tile) {
                const int ry = fold_tile == 2 ? 2 : 4, rz = fold_tile == 2 ? 4 : 2;
                const TileRows tr = tile_rows(ob.lo, ob.hi[0], b_.n[0], b_.n[1], b_.n[2], ry, rz, b_.ty);
                prof_begin(prof, "k_trans1_fold", stream);
                if (fold_tile == 2) hipLaunchKernelGGL((k_trans1_tile<0, 2, 4>), dim3(tr.nb), dim3(512), 0, stream, t, tr, S.Q, S, g, cdtdx, cdtdy, cdtdz, P);
                else hipLaunchKernelGGL((k_trans1_tile<0, 4, 2>), dim3(tr.nb), dim3(512), 0, stream, t, tr, S.Q, S, g, cdtdx, cdtdy, cdtdz, P);
                prof_end(prof, stream);
            } else
#endif
            if (n_ > 0) {
                prof_begin(prof, "k_trans1_fold", stream);
                b_.nb = fold_blocks(b_);
                hipLaunchKernelGGL(k_trans1_fold_lds<0>, dim3(b_.nb), dim3(FOLD_WG), 0, stream, t, b_, S.Q, S, g, cdtdx, cdtdy, cdtdz, P, nolv);
                prof_end(prof, stream);
            }
        } else
        KL2_SOLV("k_trans1", K_T1, plain, ob.lo, ob.hi, S.Q, S, g, cdtdx, cdtdy, cdtdz, P);
        const int assign_yz = assign_word(flags, K);
#ifdef CAD_NUMERICS_CONTRACT
        if (K.final_tile && solv == 0 && !lim) {
            constexpr int ry = 4, rz = 2;
            const TileRows tr = tile_rows(t.lo, t.hi[0], face_slots(t), t.hi[1] - t.lo[1] + 1, t.hi[2] - t.lo[2] + 1, ry, rz, K.fused_tile_rows);
            FinalOut fo;
            for (int d = 0; d < 3; ++d) { fo.fl[d] = fluxes[d]; fo.mass[d] = mass[d]; fo.qe[d] = qe[d]; fo.acc_hi[d] = acc_hi[d]; }
            prof_begin(prof, "k_final_tile", stream);
            if (clean_ntimes > 0)
                hipLaunchKernelGGL((k_final_tile<true, 0, ry, rz>), dim3(tr.nb), dim3(64 * ry * rz), 0, stream, t, tr, S.Q, S, g, Sborder, fo, Snew, dt,
                                   area0, area1, area2, vol, assign_yz, (flags & 1) ? 1 : 0, P, clean_ntimes, red);
            else
                hipLaunchKernelGGL((k_final_tile<false, 0, ry, rz>), dim3(tr.nb), dim3(64 * ry * rz), 0, stream, t, tr, S.Q, S, g, Sborder, fo, Snew, dt,
                                   area0, area1, area2, vol, assign_yz, (flags & 1) ? 1 : 0, P, 0, (double*)nullptr);
            prof_end(prof, stream);
            return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
        }
#endif
        if (lim) {
            KL2("k_final_y", (k_final<1, false, true>), plain, fb[1].lo, fb[1].hi, S.Q, S, g, Sborder, fluxes[1], mass[1], qe[1], hdtdx, hdtdz, dt, area1, g.dx[1], acc_hi[1], (flags & 2) ? 1 : 0, P, nolv);
            KL2("k_final_z", (k_final<2, false, true>), plain, fb[2].lo, fb[2].hi, S.Q, S, g, Sborder, fluxes[2], mass[2], qe[2], hdtdx, hdtdy, dt, area2, g.dx[2], acc_hi[2], (flags & 2) ? 1 : 0, P, nolv);
        } else {
            KL2_SOLV("k_final_y", K_FY, final_shape(K), fb[1].lo, fb[1].hi, S.Q, S, g, Sborder, fluxes[1], mass[1], qe[1], hdtdx, hdtdz, dt, area1, g.dx[1], acc_hi[1], assign_yz, P, nolv);
            KL2_SOLV("k_final_z", K_FZ, final_shape(K), fb[2].lo, fb[2].hi, S.Q, S, g, Sborder, fluxes[2], mass[2], qe[2], hdtdx, hdtdy, dt, area2, g.dx[2], acc_hi[2], assign_yz, P, nolv);
        }
        const XRows xr = x_rows(t, K);
        prof_begin(prof, "k_finalx_consup", stream);
#define FXC(LIM, CLEAN, GENF, nt, rd)                                                                                        \
        hipLaunchKernelGGL((k_finalx_consup<LIM, CLEAN, GENF>), dim3(xr.nb), dim3(64u * xr.wv), 0, stream, t, xr, S.Q, S, g, Sborder,      \
                           fluxes[0], mass[0], qe[0], Snew, hdtdy, hdtdz, dt, area0, area1, area2, vol, acc_hi[0],      \
                           assign_yz, (flags & 1) ? 1 : 0, P, nt, rd, nolv)
        if (clean_ntimes > 0) {
            if (lim) FXC(true, true, 2, clean_ntimes, red);
            else if (solv == 2) FXC(false, true, 2, clean_ntimes, red);
            else if (solv == 1) FXC(false, true, 1, clean_ntimes, red);
            else FXC(false, true, 0, clean_ntimes, red);
        } else {
            if (lim) FXC(true, false, 2, 0, (double*)nullptr);
            else if (solv == 2) FXC(false, false, 2, 0, (double*)nullptr);
            else if (solv == 1) FXC(false, false, 1, 0, (double*)nullptr);
            else FXC(false, false, 0, 0, (double*)nullptr);
        }
#undef FXC
        prof_end(prof, stream);
        return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
    }
    else { if (lim) TRANSVERSE_STAGES(false, true); else TRANSVERSE_STAGES(false, false); }
#undef TRANSVERSE_STAGES

    if (clean_ntimes > 0) {
        KL("k_consup_clean", k_consup<true>, plain, t.lo, t.hi, S, Sborder, Snew, dt, area0, area1, area2, vol, (flags & 1) ? 1 : 0,
           P, clean_ntimes, g.dx[0], g.dx[1], g.dx[2], red);
    } else {
        KL("k_consup", k_consup<false>, plain, t.lo, t.hi, S, Sborder, Snew, dt, area0, area1, area2, vol, (flags & 1) ? 1 : 0,
           P, 0, 0.0, 0.0, 0.0, (double*)nullptr);
    }

    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

// ---------------------------------------------------------------------------------------
// The default path for every box of a level at once (see LevelTab): 8 launches whatever the number of boxes.
// ---------------------------------------------------------------------------------------
bool level_launch_supported(const LaunchKnobs& K, const DevParams& P, int flags, bool with_src)
{
    const bool tfix = P.ppm_temp_fix == 2 && P.riemann_solver != 2;
    const bool lim = P.limit_small_dens == 1 || P.limit_large_vel == 1;
    // traced source terms (round 6): the GEN == 0 kernels read (rho e) of an edge state from its p in the `contract` build, which
    // the trace with sources promises only with CASTRO_AMD_GL_SOURCES (launch_ctu_hydro: gl_ok)
    if (with_src && gamma_law_edges(0) && !K.gl_sources) return false;
    return P.ppm_type == 1 && P.riemann_solver == 0 && P.hybrid_riemann != 1 && !tfix && P.reset_rhoe != 1 && !lim &&
           K.fuse_consup == 1 && K.fold_r1 != 0 && (flags & (4 | 8 | 16 | 32 | 64)) == 0;
}

int launch_ctu_hydro_level(const LaunchKnobs& K, int nbox, const LevelBoxDesc* boxes, StagedTable* table, const DevGeom& g, const DevParams& P,
                           double dt, int flags, int* d_status, hipStream_t stream, Profiler* prof, int clean_ntimes, double* red, int sb_clean)
{
    if (nbox < 1 || !boxes || !table) return CASTRO_AMD_ERR_ARG;
    // Traced source terms: every box of the launch has its old-time source FAB or none has.  The sequence is launch_ctu_hydro's
    // for Src.p != nullptr -- k_divu_pair, k_src_to_prim, the one-zone trace with sources, the first x solves as a launch of
    // their own -- through the table forms of those kernels; the transverse and final stages are the same either way.
    const bool with_src = boxes[0].Src.p != nullptr;
    for (int i = 1; i < nbox; ++i) if ((boxes[i].Src.p != nullptr) != with_src) return CASTRO_AMD_ERR_ARG;
    if (with_src && sb_clean > 0) return CASTRO_AMD_ERR_ARG;
    const Shape plain = plain_shape(K);
    std::vector<LevelBox> hb((size_t)nbox);
    std::vector<unsigned> start((size_t)NLB * (size_t)(nbox + 1), 0u);
    auto st = [&](int kind, int i) -> unsigned& { return start[(size_t)kind * (size_t)(nbox + 1) + (size_t)i]; };
    for (int i = 0; i < nbox; ++i) {
        const LevelBoxDesc& D = boxes[i];
        LevelBox& B = hb[(size_t)i];
        const Tile& t = D.t;
        B.t = t; B.S = D.S; B.U = D.U; B.Unew = D.Unew; B.Src = D.Src;
        for (int d = 0; d < 3; ++d) { B.fl[d] = D.fl[d]; B.mass[d] = D.mass[d]; B.qe[d] = D.qe[d]; B.acc_hi[d] = D.acc_hi[d]; }
        // every box in the shape launch_ctu_hydro gives the same launch
        const SkipBox ob = grow(t, 1), qb = grow(t, 4);
        long n_;
        B.b[LB_CTOPRIM] = linbox(qb.lo, qb.hi, plain, n_);
        B.b[LB_DIVU] = linbox2(ob.lo, ob.hi, plain, n_);
        B.b[LB_TRACE] = linbox2(ob.lo, ob.hi, trace_shape(K), n_);
        B.b[LB_FOLD] = linbox2(ob.lo, ob.hi, fold_shape(K), n_);
        B.b[LB_FOLD].nb = fold_blocks(B.b[LB_FOLD]);
        for (int m = 0; m < 3; ++m) { B.bs[m] = LinBox{}; B.bs[m].nb = 0; }
        if (with_src) {
            const SkipBox q3 = grow(t, 3), f0 = face_box(t, 0, 1);
            B.bs[0] = linbox(q3.lo, q3.hi, plain, n_);
            B.bs[1] = linbox(ob.lo, ob.hi, plain, n_);
            B.bs[2] = linbox2(f0.lo, f0.hi, plain, n_);
        }
        for (int d = 1; d <= 2; ++d) {
            const SkipBox fb = face_box(t, d, 0);
            B.b[d == 1 ? LB_FY : LB_FZ] = linbox2(fb.lo, fb.hi, final_shape(K), n_);
        }
        B.xr = x_rows(t, K);
        const XRows& xr = B.xr;
        // workgroup ranges: multiples of 8 wherever the kernel maps ids to XCDs (every LinBox with ty > 0 is one already)
        const unsigned nbs[NLB] = { B.b[LB_CTOPRIM].nb, B.b[LB_DIVU].nb, B.b[LB_TRACE].nb, B.b[LB_FOLD].nb, B.b[LB_FY].nb, B.b[LB_FZ].nb,
                                    xr.nb, (B.b[LB_TRACE].nb + 255u) / 256u, B.bs[0].nb, B.bs[1].nb, B.bs[2].nb };
        for (int kind = 0; kind < NLB; ++kind) {
            unsigned nb = nbs[kind];
            if (kind != LB_BSTART) nb = (nb + 7u) & ~7u;
            st(kind, i + 1) = st(kind, i) + nb;
        }
    }
    // the table: boxes, then the prefix arrays
    const LevelBox* dbox;
    const unsigned* dstart;
    const int rt = table->stage(hb.data(), hb.size(), start.data(), start.size(), stream, dbox, dstart);
    if (rt != 0) return rt;
    auto lv = [&](int kind) { return LevelTab{ dbox, dstart + (size_t)kind * (size_t)(nbox + 1), nbox }; };
    auto total = [&](int kind) { return st(kind, nbox); };

    const Tile t0 = hb[0].t;
    const DevScratch S0 = hb[0].S;
    const SkipBox none = { { 0, 0, 0 }, { -1, -1, -1 } };
    const int assign = assign_word(flags, K);
    const auto [cdtdx, cdtdy, cdtdz, hdtdx, hdtdy, hdtdz, area0, area1, area2, vol] = step_consts(g, dt);

    prof_begin(prof, sb_clean > 0 ? "k_ctoprim_clean" : "k_ctoprim", stream);
    if (sb_clean > 0) hipLaunchKernelGGL((k_ctoprim<true, true>), dim3(total(LB_CTOPRIM)), dim3(hb[0].b[LB_CTOPRIM].wg), 0, stream, t0, hb[0].b[LB_CTOPRIM],
                                         hb[0].U, S0.Q, P, d_status, none, sb_clean, lv(LB_CTOPRIM), gamma_law_edges(0) ? (clean_ntimes > 0 ? 3 : 1) : 0, 0, ShellBoxes{}, BcKinds{});
    else hipLaunchKernelGGL((k_ctoprim<false, true>), dim3(total(LB_CTOPRIM)), dim3(hb[0].b[LB_CTOPRIM].wg), 0, stream, t0, hb[0].b[LB_CTOPRIM],
                            hb[0].U, S0.Q, P, d_status, none, 0, lv(LB_CTOPRIM), gamma_law_edges(0) ? (clean_ntimes > 0 ? 3 : 1) : 0, 0, ShellBoxes{}, BcKinds{});
    prof_end(prof, stream);
    if (!K.divu_in_trace || with_src) {
        prof_begin(prof, "k_divu", stream);
        hipLaunchKernelGGL(k_divu_pair<true>, dim3(total(LB_DIVU)), dim3(hb[0].b[LB_DIVU].wg), 0, stream, t0, hb[0].b[LB_DIVU], S0.Q, S0.DIV,
                           1.0 / g.dx[0], 1.0 / g.dx[1], 1.0 / g.dx[2], lv(LB_DIVU));
        prof_end(prof, stream);
    }
    if (with_src) {
        const int lean = gamma_law_edges(0) ? 1 : 0;          // launch_ctu_hydro's lean_q & 1 on this path (solv == 0)
        prof_begin(prof, "k_src_to_prim", stream);
        hipLaunchKernelGGL(k_src_to_prim<true>, dim3(total(LB_SRCPRIM)), dim3(hb[0].bs[0].wg), 0, stream, t0, hb[0].bs[0], S0.Q, hb[0].Src, S0.SRCQ, P,
                           DFab{ nullptr, { 0, 0, 0 }, 0, 0, 0 }, dt, lean, lv(LB_SRCPRIM));
        prof_end(prof, stream);
        prof_begin(prof, "k_trace", stream);
        hipLaunchKernelGGL((k_trace<true, false, gamma_law_edges(0), true>), dim3(total(LB_TRACE1)), dim3(hb[0].bs[1].wg), 0, stream, t0, hb[0].bs[1], S0.Q, S0, g,
                           dt, P, lv(LB_TRACE1));
        prof_end(prof, stream);
        prof_begin(prof, "k_riemann1", stream);
        hipLaunchKernelGGL((k_riemann1<0, false, 0, true>), dim3(total(LB_R1X)), dim3(hb[0].bs[2].wg), 0, stream, t0, hb[0].bs[2], S0.Q, S0, g, P, lv(LB_R1X));
        prof_end(prof, stream);
    } else {
    prof_begin(prof, "k_trace", stream);
    hipLaunchKernelGGL((k_trace_pair<true, 7, 0, true>), dim3(total(LB_TRACE)), dim3(hb[0].b[LB_TRACE].wg), 0, stream, t0, hb[0].b[LB_TRACE], S0.Q, S0, g,
                       dt, P, none, lv(LB_TRACE), K.divu_in_trace ? 1 : 0);
    prof_end(prof, stream);
    prof_begin(prof, "k_riemann1_blockstart", stream);
    hipLaunchKernelGGL((k_riemann1_blockstart<0, true>), dim3(total(LB_BSTART)), dim3(256), 0, stream, t0, hb[0].b[LB_TRACE], S0.Q, S0, g, P, lv(LB_BSTART));
    prof_end(prof, stream);
    }
    prof_begin(prof, "k_trans1_fold", stream);
    hipLaunchKernelGGL((k_trans1_fold_lds<0, true>), dim3(total(LB_FOLD)), dim3(FOLD_WG), 0, stream, t0, hb[0].b[LB_FOLD], S0.Q, S0, g, cdtdx, cdtdy, cdtdz, P,
                       lv(LB_FOLD));
    prof_end(prof, stream);
    prof_begin(prof, "k_final_y", stream);
    hipLaunchKernelGGL((k_final<1, false, false, 0, true>), dim3(total(LB_FY)), dim3(hb[0].b[LB_FY].wg), 0, stream, t0, hb[0].b[LB_FY], S0.Q, S0, g, hb[0].U,
                       hb[0].fl[1], hb[0].mass[1], hb[0].qe[1], hdtdx, hdtdz, dt, area1, g.dx[1], hb[0].acc_hi[1], assign, P, lv(LB_FY));
    prof_end(prof, stream);
    prof_begin(prof, "k_final_z", stream);
    hipLaunchKernelGGL((k_final<2, false, false, 0, true>), dim3(total(LB_FZ)), dim3(hb[0].b[LB_FZ].wg), 0, stream, t0, hb[0].b[LB_FZ], S0.Q, S0, g, hb[0].U,
                       hb[0].fl[2], hb[0].mass[2], hb[0].qe[2], hdtdx, hdtdy, dt, area2, g.dx[2], hb[0].acc_hi[2], assign, P, lv(LB_FZ));
    prof_end(prof, stream);
    prof_begin(prof, "k_finalx_consup", stream);
    if (clean_ntimes > 0)
        hipLaunchKernelGGL((k_finalx_consup<false, true, 0, true>), dim3(total(LB_FX)), dim3(64u * hb[0].xr.wv), 0, stream, t0, hb[0].xr, S0.Q, S0, g, hb[0].U,
                           hb[0].fl[0], hb[0].mass[0], hb[0].qe[0], hb[0].Unew, hdtdy, hdtdz, dt, area0, area1, area2, vol, hb[0].acc_hi[0],
                           assign, (flags & 1) ? 1 : 0, P, clean_ntimes, red, lv(LB_FX));
    else
        hipLaunchKernelGGL((k_finalx_consup<false, false, 0, true>), dim3(total(LB_FX)), dim3(64u * hb[0].xr.wv), 0, stream, t0, hb[0].xr, S0.Q, S0, g, hb[0].U,
                           hb[0].fl[0], hb[0].mass[0], hb[0].qe[0], hb[0].Unew, hdtdy, hdtdz, dt, area0, area1, area2, vol, hb[0].acc_hi[0],
                           assign, (flags & 1) ? 1 : 0, P, 0, (double*)nullptr, lv(LB_FX));
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

} // namespace cad

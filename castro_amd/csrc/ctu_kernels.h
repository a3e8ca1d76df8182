// ctu_kernels.h -- host/device shared descriptors of the HIP CTU hydro path.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "hydro_device.h"
#include "dev_table.h"

struct castro_amd_rotation;      // include/castro_hydro_amd.h
struct castro_amd_sponge;
struct castro_amd_ext_bc;
struct castro_amd_geom;

namespace cad {

// one tile of work: bx = [lo,hi]; every scratch array is indexed on grow(bx,4)
struct Tile {
    int lo[3], hi[3];
    int glo[3];
    int NX, NY, NZ;
    long NC;       // doubles per component plane (>= NX*NY*NZ, padded for alignment)
};

// caller-owned FArrayBox on the device
struct DFab {
    double* p;
    int lo[3];
    long sy, sz, sn;
};

struct DevGeom {
    double dx[3];
    int domlo[3], domhi[3];
    int wall_lo[3], wall_hi[3];   // Symmetry / SlipWall / NoSlipWall: zero normal flux (riemann.cpp:53-59)
    int sym_lo[3], sym_hi[3];     // Symmetry only: PLM reflecting treatment (trace_plm.cpp:39-40, Castro_ctu.cpp:293-294)
};

struct DevScratch {
    double* Q;        // NPRIM planes
    double* DIV;      // 1 plane
    double* SHK;      // 1 plane (hybrid Riemann only)
    double* SRCQ;     // 6 planes (rho,u,v,w,p,rhoe primitive sources; only with a source FAB)
    double* QM[3];    // NEDGE planes each
    double* QP[3];
    double* F1[3];    // NF1 planes each
    double* F2[6];    // NF1 planes each, slot f2_slot(N,T)
    double* FL[3];    // NFIN planes each
    double* F1E[3];   // (rho e) flux of the first solves, 1 plane each -- written and read only with transverse_reset_rhoe = 1
    double* F2E[6];   // the same for the transverse-stage solves
};

// hipEvent-based per-kernel timing (enabled on request only: it serialises nothing, the
// events are recorded on the same stream as the kernels)
struct Profiler {
    struct Rec { std::string name; double total_ms = 0.0; long long launches = 0; };
    bool enabled = false;
    std::vector<Rec> recs;
    struct Pending { int rec; hipEvent_t e0, e1; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    int cur = -1;
    hipEvent_t cur_e0{}, cur_e1{};
};
void prof_begin(Profiler* p, const char* name, hipStream_t s);
void prof_end(Profiler* p, hipStream_t s);
void prof_collect(Profiler* p);

// Launch forms and launch geometry of the hydro path.  A context reads them from the environment when it is created
// (launch_knobs_from_env) and never writes them again: they hold for that context only, whatever is created beside it.
struct LaunchKnobs {
    int tile_rows = 32;         // CASTRO_AMD_TILE_ROWS: 0 = plain row-major workgroup order; > 0 = XCD-tiled order with this many rows per y-tile
    int trace_tile_rows = 64;   // CASTRO_AMD_TRACE_TILE_ROWS: rows per y-tile of the trace launch and its block-start fix-up (its L2 holds
                                // only Q now that the stores are non-temporal: 2.72 -> 2.60 ms; -1: tile_rows)
    int fold_tile_rows = -1;    // CASTRO_AMD_FOLD_TILE_ROWS: rows per y-tile of the k_trans1_fold launch (-1: tile_rows)
    int fused_tile_rows = 16;   // CASTRO_AMD_FUSED_TILE_ROWS: rows per y-tile of the k_finalx_consup row order (0: plain)
    int wg = 256;               // CASTRO_AMD_WG: threads per workgroup of every launch built from a LinBox (64, 128 or 256)
    int final_wg = 0;           // CASTRO_AMD_FINAL_WG: k_final<y>, k_final<z> only (0: wg)
    int fused_wg = 128;         // CASTRO_AMD_FUSED_WG: k_finalx_consup (its waves share nothing: 2.16-2.20 ms at 256, 2.04-2.05 at 128 / 64
                                // threads, profiles/r03x_*)
    int xpad = 0;               // CASTRO_AMD_XPAD: unused columns in front of every scratch row (capi.hip: scratch_nx)
    int fuse_consup = 1;        // CASTRO_AMD_FUSE_CONSUP: 1 = k_finalx_consup (the x faces of the final stage and consup_hydro in one
                                // kernel), 0 = k_final<x> + k_consup
    int fold_r1 = 2;            // CASTRO_AMD_FOLD_R1: the first y / z Riemann solves inside the transverse stage: != 0 = k_trans1_fold_lds
                                // (records parked in LDS; -0.35 ms per 256^3 step), 0 = two k_riemann1 launches + k_trans1 (profiles/r03c_*, r03d_*)
    int fold_tile = -1;         // CASTRO_AMD_FOLD_TILE: 1 = k_trans1_tile<4, 2> (a 4 x 2 tile of rows per workgroup), 2 = <2, 4>,
                                // 0 = k_trans1_fold_lds; -1: <4, 2> for boxes of at least 96 rows in y and z (128^3: equal, 64^3: the fold
                                // kernel is faster; profiles/r05c_ab_fold_tile_kernel.txt); `contract` build only
    int final_tile = 0;         // CASTRO_AMD_FINAL_TILE: 1 = the final stage as ONE zone-centred launch (k_final_tile<4, 2>); `contract` build only
    int gl_sources = 1;         // CASTRO_AMD_GL_SOURCES: 0 = traced source terms run the 7-variable kernels as in round 4 (A/B)
    int gl_plm = 1;             // CASTRO_AMD_GL_PLM: 0 = the PLM trace (ppm_type = 0) runs the 7-variable kernels as before round 6 (A/B)
    // CASTRO_AMD_DIVU_IN_TRACE: div(u) inside k_trace_pair instead of a k_divu_pair launch of its own.  `contract`: on (-0.08 ms per
    // 256^3 step, -0.02 ms at 128^3: the launch of 0.18 ms becomes 0.09 ms more trace); `exact`: off (its trace kernel sits at
    // 252 VGPRs: +0.1 ms).  profiles/r06j_*
#ifdef CAD_NUMERICS_CONTRACT
    int divu_in_trace = 1;
#else
    int divu_in_trace = 0;
#endif
    int trace_one_zone = 0;     // CASTRO_AMD_TRACE_ONE_ZONE: 1 = k_trace (one zone per thread) + k_riemann1<x> instead of k_trace_pair: an
                                // occupancy A/B, slower
    int side_stream = 0;        // CASTRO_AMD_SIDE_STREAM: 1 = k_divu runs on the context's side stream beside the trace kernel; measured: no
                                // gain, two independent pipelines on two streams take as long as one after the other (tools/concurrency_probe.py)
    int lazy_loads = 1;         // CASTRO_AMD_LAZY_LOADS: the final kernels load what the update discards in almost every zone only where it is
                                // kept: the old state of apply_av on compressive faces (`contract` build), the operands of the evolved (rho e)
                                // where reset_internal_energy keeps it.  0 = every zone loads them (A/B in one binary; same bits in S_new);
                                // 2 / 3 = the first / the second of the two alone
};
// the variables above as the environment has them now; one that is not set gives the default
LaunchKnobs launch_knobs_from_env();

// what a call carries besides its arrays: the context's knobs, in-place cleaning of Sborder inside k_ctoprim, the context's side stream
struct LaunchAux {
    LaunchKnobs knobs;
    int sb_clean = 0;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int bc_lo[3] = { 0, 0, 0 }, bc_hi[3] = { 0, 0, 0 };     // castro_amd_geom::lo_bc / hi_bc (CASTRO_AMD_BC_FILL)
};

int launch_ctu_hydro(const Tile& t, const DevScratch& S, const DFab& Sborder, const DFab& Src, const DFab& Snew,
                     const DFab fluxes[3], const DFab mass[3], const DFab qe[3],
                     const DevGeom& g, const DevParams& P, double dt, int flags, const int acc_hi[3],
                     int* d_status, hipStream_t stream, Profiler* prof, int clean_ntimes, double* red, const DFab& SrcCorr,
                     const LaunchAux& aux);

// One box of a level-wide launch (castro_amd_ctu_hydro_mf): its tile, its own scratch, the caller's arrays
struct LevelBoxDesc {
    Tile t;
    DevScratch S;
    DFab U, Unew, fl[3], mass[3], qe[3];
    int acc_hi[3];
    DFab Src;              // old-time source FAB to be traced (p == nullptr: none); all boxes of a launch alike
};
// default options only (PPM, CGF solver, no staging, the default kernel forms; traced source terms without a predictor): else box by box
// K: the knobs of the context whose prepare_box laid out the boxes' scratch
bool level_launch_supported(const LaunchKnobs& K, const DevParams& P, int flags, bool with_src = false);
int launch_ctu_hydro_level(const LaunchKnobs& K, int nbox, const LevelBoxDesc* boxes, StagedTable* table, const DevGeom& g, const DevParams& P,
                           double dt, int flags, int* d_status, hipStream_t stream, Profiler* prof, int clean_ntimes, double* red, int sb_clean);

// auxiliary per-FAB kernels (aux_kernels.hip)
int launch_clean_state(const DFab& U, const int lo[3], const int hi[3], const DevParams& P, int ntimes,
                       hipStream_t stream, Profiler* prof);
int launch_clean_state_reduce(const DFab& U, const int lo[3], const int hi[3], const DevGeom& g, const DevParams& P,
                              int ntimes, double* d_out, hipStream_t stream, Profiler* prof);
int launch_step_control(double* red, double* ctl, double cfl, double change_max, double small_dens, double max_dt,
                        double fixed_dt, double stop_time, int retry_form, hipStream_t stream, Profiler* prof);
int launch_estdt(const DFab& U, const int lo[3], const int hi[3], const DevGeom& g, const DevParams& P,
                 double* d_out, hipStream_t stream, Profiler* prof);
int launch_old_grav_source(const DFab& U, const DFab& SRC, const int lo[3], const int hi[3], const double grav[3],
                           int type, double dt, hipStream_t stream, Profiler* prof);
int launch_new_grav_source(const DFab& UO, const DFab& UN, const DFab& SRC, const DFab M[3], const int lo[3], const int hi[3],
                           const double grav[3], int type, double dt, const double dx[3], hipStream_t stream, Profiler* prof);
int launch_old_rot_source(const DFab& U, const DFab& SRC, const int lo[3], const int hi[3], const ::castro_amd_rotation* r,
                          const ::castro_amd_geom* g, double dt, hipStream_t stream, Profiler* prof);
int launch_new_rot_source(const DFab& UO, const DFab& UN, const DFab& SRC, const DFab M[3], const int lo[3], const int hi[3],
                          const ::castro_amd_rotation* r, const ::castro_amd_geom* g, double dt, hipStream_t stream, Profiler* prof);
// the sponge (Castro_sponge.cpp): a new-time source made from S_new alone, added to UMX..UMZ and UEDEN of SRC on [lo, hi]
int launch_new_sponge_source(const DFab& UN, const DFab& SRC, const int lo[3], const int hi[3], const ::castro_amd_sponge* s,
                             const ::castro_amd_geom* g, const DevParams& P, double dt, hipStream_t stream, Profiler* prof);
// one box of castro_amd_sources_mf: states, Source_Type FAB (nsc components), mass fluxes; [lo, lo + n): the zones of the source FAB
// (thread range), [vlo, vhi]: the valid zones
struct SrcBoxDev { DFab So, Sn, Src, M0, M1, M2; int lo[3], n[3]; int vlo[3], vhi[3]; int nsc; };
// one box of castro_amd_sources_mf_g: the same, and its Gravity_Type FABs (3 components, one ghost zone around [vlo, vhi])
struct SrcBoxGDev { SrcBoxDev box; DFab GO, GN; };
int launch_sources_apply_gfab(int stage, int nbox, const SrcBoxGDev* boxes, int grav_type, const ::castro_amd_rotation* rot,
                              const ::castro_amd_geom* geom, const DevParams& P, double dt, int ntimes, StagedTable* arena,
                              hipStream_t stream, Profiler* prof, int diff_on = 0, const ::castro_amd_sponge* sponge = nullptr);
int launch_sources_apply(int stage, int nbox, const SrcBoxDev* boxes, const double* grav, int grav_type, const ::castro_amd_rotation* rot,
                         const ::castro_amd_geom* geom, const DevParams& P, double dt, int ntimes, StagedTable* arena,
                         hipStream_t stream, Profiler* prof, int diff_on = 0, const ::castro_amd_sponge* sponge = nullptr);
// thermal diffusion (diffusion_kernels.hip).  One box of a castro_amd_temp_diffusion_* launch: U (and U2, the old state of the
// time-centred corrector) with at least one ghost zone around [lo, hi]; Src: the Source_Type FAB (p == nullptr: none);
// Out: a one-component FAB for the bare term (p == nullptr: none); nt: tiles per direction, set by the launcher
struct DiffBoxDev { DFab U, U2, Src, Out; int lo[3], hi[3], nt[3]; };
// phys_lo / phys_hi: the domain face of that direction is a physical boundary (zero flux) rather than periodic
struct DiffDev { double cond, cutoff, cutoff_hi, scale; double dh[3]; int domlo[3], domhi[3]; int phys_lo[3], phys_hi[3]; };
int launch_temp_diffusion(int nbox, DiffBoxDev* boxes, bool two, const DiffDev& D, double m1, double m2, int init,
                          StagedTable* arena, hipStream_t stream, Profiler* prof);
int launch_estdt_temp_diffusion(const DFab& U, const int lo[3], const int hi[3], const double dx[3], const DevParams& P,
                                double cond, double cutoff, double below, double* d_out, hipStream_t stream, Profiler* prof);
// integrated quantities (diag_kernels.hip).  One box of a castro_amd_integrated_quantities_mf launch: the valid zones
// [lo, lo + n) of U, the byte mask of those zones (nullptr: every zone counts); npr: pairs of x-adjacent zones per row, set by
// diag_layout
struct DiagBoxDev { DFab U; const unsigned char* mask; int lo[3], n[3]; int npr; };
struct DiagGeom { double dx[3], problo[3], center[3], vol; };
// rows of partial sums of the context: reserved at first use, grown only by a launch with more workgroups than any before
struct DiagWorkspace { double* p = nullptr; size_t rows = 0; };
// start[r]: first workgroup of box r (start[nbox]: all of them); iters: pairs a thread takes.  Returns 0 or CASTRO_AMD_ERR_ARG
int diag_layout(int nbox, DiagBoxDev* boxes, std::vector<int>& start, int& iters);
int launch_integrated_quantities(int nbox, DiagBoxDev* boxes, const DiagGeom& G, StagedTable* arena, DiagWorkspace* ws,
                                 double* d_out, hipStream_t stream, Profiler* prof);
// checkpoints (checkpoint_kernels.hip).  One entry of a castro_amd_fab_pack / _unpack launch: p -> the first valid zone of component
// 0, the strides of the FAB in doubles, n: the extent of the valid region, zones = n[0] n[1] n[2], offset: where the region starts
// in the buffer; vec2: a lane moves two zones per access (every row starts on a 16-byte boundary on both sides), items: zones or
// pairs per component; bpc: workgroups per component, set by the launcher
struct PackEntryDev { double* p; long sy, sz, sn, offset, zones, items; int n[3]; int ncomp, bpc, vec2; };
// mode 0: pack (d_minmax or nullptr), 1: unpack; ws: one (min, max) pair per workgroup
int launch_fab_pack(int mode, int n, PackEntryDev* tab, StagedTable* arena, DiagWorkspace* ws, double* buf, double* d_minmax,
                    hipStream_t stream, Profiler* prof);
// monopole gravity (monopole_kernels.hip).  One box of a castro_amd_radial_mass_mf launch: the valid zones [lo, lo + n) of U, the
// byte mask of those zones (nullptr: every zone counts); nb: bricks per direction, set by the launcher.  A table is compared
// byte by byte with the ones the context has on the device: fill it field by field over zeroed storage
struct MonoBoxDev { DFab U; const unsigned char* mask; int lo[3], n[3], nb[3]; };
// one box of a castro_amd_radial_mass_mf_ex launch: MonoBoxDev's fields in MonoBoxDev's order, then the new-time state and the
// weights of the time interpolation, rho = (U(URHO) * omalpha) + (U2(URHO) * alpha)
struct MonoBoxDevEx { DFab U; const unsigned char* mask; int lo[3], n[3], nb[3]; DFab U2; double omalpha, alpha; };
// castro_amd_radial_combine: the mass / volume arrays (2 * n1d[lev] doubles each) of levels 0 .. level
constexpr int MONO_MAX_LEVELS = 16;
struct MonoCombine { const double* mv[MONO_MAX_LEVELS]; int n1d[MONO_MAX_LEVELS]; int level; };
// octant_factor: 8 when the centre sits on problo (Gravity.cpp:1439-1447), else 1; max_radius: max_radius_all_in_domain
struct MonoGeom { double dx[3], problo[3], center[3]; double octant_factor, max_radius, Gconst; int n1d, drdxfac; };
// what a context keeps for the binning: one row of 64 bins and its first bin per workgroup, the integer counts per bin, and the
// box tables it has copied to the device (dev_table.h).  Reserved at first use; grown only by a call with more workgroups,
// more bins or a table not seen before -- any other call neither allocates nor synchronises
struct MonoWorkspace {
    double* rows = nullptr; int* rbase = nullptr; size_t nrows = 0;
    unsigned long long* count = nullptr; size_t ncount = 0;
    TableCache tables{8};
};
bool radial_window_ok(const MonoGeom& G);
void mono_workspace_free(MonoWorkspace* ws);
int launch_radial_mass(int nbox, MonoBoxDev* boxes, const MonoGeom& G, MonoWorkspace* ws, double* d_out, hipStream_t stream,
                       Profiler* prof);
int launch_radial_mass_ex(int nbox, MonoBoxDevEx* boxes, const MonoGeom& G, MonoWorkspace* ws, double* d_out, hipStream_t stream,
                          Profiler* prof);
int launch_radial_combine(const MonoCombine& A, double* d_out, hipStream_t stream, Profiler* prof);
// Gravity_Type boundary fill of the zones of [flo, fhi] outside the domain (3 components)
int launch_grav_bc_fill(const DFab& F, const int flo[3], const int fhi[3], const int domlo[3], const int domhi[3],
                        const int lo_bc[3], const int hi_bc[3], hipStream_t stream, Profiler* prof);
int launch_radial_gravity(const MonoGeom& G, const double* d_mass_vol, double* d_radial_grav, hipStream_t stream, Profiler* prof);
int launch_monopole_grav(const double* d_radial_grav, const MonoGeom& G, const DFab& F, const int lo[3], const int hi[3],
                         hipStream_t stream, Profiler* prof);
// Poisson gravity (poisson_kernels.hip).  One level of the multigrid: its box [lo, lo + n), cx = 1 / (hx hx) ... and
// cdiag = 2 ((cx + cy) + cz), formed on the host (poisson_levels) so that a restatement can form the same bits
constexpr int MG_MAX_LEVELS = 32;
constexpr int MG_NPRE = 2, MG_NPOST = 2, MG_NBOTTOM = 32;      // red-black sweeps before / after the coarser levels, and of the bottom solve
struct MgLevel { int n[3], lo[3]; double cx, cy, cz, cdiag; };
// what a plan owns: the levels, the arrays of every level (phi[0] is the caller's FAB, set per solve; the ghost zones of the
// coarser phi stay zero), two device norms per reduction, the workgroup maxima behind them and a pinned host copy
struct PoissonPlan {
    std::vector<MgLevel> lev;
    std::vector<DFab> phi, rhs, res;
    std::vector<double*> owned;
    double dx[3];
    double* d_norm = nullptr; double* norm_ws = nullptr; double* h_norm = nullptr;
    // a plan of a union of boxes (poisson_boxes_plan_make; empty otherwise): lev[m] is the bounding box >> m, flags[m] one byte
    // per zone of it (MGF_*, x fastest), boxes the union in the zones of level 0 (lo, hi: 6 ints per box), and the box tables
    // of the right-hand side and of the gradient the plan has copied to the device
    std::vector<unsigned char*> flags;
    std::vector<int> boxes;
    TableCache tables{8};
};
// flags of a zone of a union of boxes: covered, and "the neighbour across this face is not covered" for the face (d, side)
constexpr unsigned MGF_COVERED = 1u;
constexpr unsigned mgf_face(int d, int side) { return 2u << (2 * d + side); }
// one box of the union with its own FAB (the state, or Gravity_Type data): thread range [start, start + n[0] n[1] n[2])
struct MgBoxDev { DFab F; int lo[3], n[3]; long start; };
int poisson_boxes_levels(int nbox, const int* lo, const int* hi, const double dx[3], std::vector<MgLevel>& lev);
int poisson_boxes_plan_make(int nbox, const int* lo, const int* hi, const double dx[3], PoissonPlan** out);
// The edge of a level, as the launchers of the passes take it.  flags == nullptr: the level is the one box of L, the values on
// its faces are in the ghost zones of phi.  Otherwise the flags of a union of boxes and X, the face values of level 0 (3
// components over the bounding box with its high corner grown by one: component d at the zone (i, j, k) is the low d-face of
// that zone); X.p == nullptr: every face value is 0.0 (the coarser levels)
struct MgEdge { const unsigned char* flags; DFab X; };
// U: the state FAB of every box of the plan, in the plan's order
int launch_poisson_boxes_solve(PoissonPlan* P, const DFab& phi, const DFab& X, const DFab* U, int comp, double fourpiG, double reltol,
                               double abstol, int maxiter, int* cycles, int* converged, double* final_norm, double* h_history,
                               hipStream_t s, Profiler* prof);
int launch_grad_phi_boxes(PoissonPlan* P, const DFab& phi, const DFab& X, const DFab* G, hipStream_t s, Profiler* prof);
int launch_phi_cf_boxes(PoissonPlan* P, const DFab& X, const DFab& O, const DFab& N, double a, hipStream_t s, Profiler* prof);
int poisson_levels(const int n[3], const int lo[3], const double dx[3], std::vector<MgLevel>& lev);
int poisson_plan_make(const int n[3], const int lo[3], const double dx[3], PoissonPlan** out);
void poisson_plan_free(PoissonPlan* P);
int launch_mg_smooth(const DFab& P, const DFab& B, const MgLevel& L, const MgEdge& e, int colour, hipStream_t s, Profiler* prof);
int launch_mg_residual(const DFab& P, const DFab& B, const DFab& R, const MgLevel& L, const MgEdge& e, hipStream_t s, Profiler* prof);
int launch_mg_restrict(const DFab& RF, const MgLevel& LF, const DFab& BC, const DFab& PC, const MgLevel& LC, const unsigned char* cflags,
                       hipStream_t s, Profiler* prof);
int launch_mg_prolong(const DFab& PC, const MgLevel& LC, const DFab& PF, const MgLevel& LF, const unsigned char* fflags, hipStream_t s,
                      Profiler* prof);
int launch_mg_norm(const DFab& X, const MgLevel& L, const unsigned char* flags, double* ws, double* d_out, hipStream_t s, Profiler* prof);
// h_history (or nullptr): ||b||, max b, the norm of the starting residual, then the norm after every cycle (maxiter + 3 doubles)
int launch_poisson_solve(PoissonPlan* P, const DFab& phi, const DFab& U, int comp, double fourpiG, double reltol, double abstol,
                         int maxiter, int* cycles, int* converged, double* final_norm, double* h_history, hipStream_t s, Profiler* prof);
int launch_grad_phi(const DFab& phi, const DFab& G, const MgLevel& L, const double dx[3], hipStream_t s, Profiler* prof);
struct MpGeom { double dx[3], problo[3], center[3]; double rmax, Gconst; int lnum; int domlo[3], domhi[3]; };
// d_out: 3 (lnum + 1)^2 doubles, [kind][l][m], kind 0 = qL0 (m = 0), 1 = qLC, 2 = qLS; ws: rows of MP_NC doubles
int launch_multipole_moments(int nbox, DiagBoxDev* boxes, const MpGeom& G, StagedTable* arena, DiagWorkspace* ws, double* d_out,
                             hipStream_t stream, Profiler* prof);
// the central point mass (pointmass_kernels.hip).  One gravity FAB of a castro_amd_add_pointmass_* launch: its whole box
// [lo, lo + n), ghost zones included; start: the first thread of the FAB, set by the launcher.  One box of a
// castro_amd_pointmass_delta_mf / _apply_mf launch: the valid zones [lo, hi] of the old and the new state.  Both tables are
// compared byte by byte with the ones the context has on the device: fill them field by field over zeroed storage
struct PmFabDev { DFab F; int lo[3], n[3]; long start; };
struct PmBoxDev { DFab So, Sn; int lo[3], hi[3]; };
struct PmGeom { double dx[3], problo[3], center[3]; double Gconst; };
int launch_add_pointmass(int nfab, PmFabDev* fabs, const PmGeom& G, const double* d_mass, TableCache* tables, hipStream_t stream,
                         Profiler* prof);
// clo: the low corner of the 4 x 4 x 4 cube (icen - 2 of Castro_pointmass.cpp:43-65)
int launch_pointmass_delta(int nbox, const PmBoxDev* boxes, const int clo[3], double vol, double* d_delta, TableCache* tables,
                           hipStream_t stream, Profiler* prof);
int launch_pointmass_apply(int nbox, const PmBoxDev* boxes, const int clo[3], const double* d_delta, double* d_mass,
                           TableCache* tables, hipStream_t stream, Profiler* prof);
// tracer particles (tracer_kernels.hip).  One box of a level: the FAB (count: its int32 zones behind F.p), the box of the array
// [alo, ahi] and the valid box [vlo, vhi].  Compared byte by byte like the tables above: fill over zeroed storage.
// TrGeom: advect / sample / count read dxi[0] (the level's own), locate dxi[l] and the boxes tab[start[l], start[l + 1]) of level l
#define CAD_TRACER_MAX_LEVELS 16
struct TrBoxDev { DFab F; int alo[3], ahi[3], vlo[3], vhi[3]; };
struct TrGeom { double plo[3], phi[3]; int periodic[3]; int nlev; int start[CAD_TRACER_MAX_LEVELS + 1]; double dxi[CAD_TRACER_MAX_LEVELS][3]; };
struct TrComps { int n; int comp[CASTRO_AMD_NUM_STATE]; };
int launch_tracer_advect(int nbox, const TrBoxDev* boxes, int level, const TrGeom& G, double dt, int ipass, const castro_amd_tracers& T,
                         int* d_flags, TableCache* tables, hipStream_t stream, Profiler* prof);
int launch_tracer_sample(int nbox, const TrBoxDev* boxes, int level, const TrGeom& G, const TrComps& C, const castro_amd_tracers& T,
                         double* d_out, int* d_flags, TableCache* tables, hipStream_t stream, Profiler* prof);
int launch_tracer_locate(int nbox, const TrBoxDev* boxes, const TrGeom& G, int lev_min, int lev_max, int ngrow,
                         const castro_amd_tracers& T, int* d_flags, TableCache* tables, hipStream_t stream, Profiler* prof);
int launch_tracer_count(int nbox, const TrBoxDev* boxes, int level, const TrGeom& G, const castro_amd_tracers& T, TableCache* tables,
                        hipStream_t stream, Profiler* prof);
// migration between ranks.  TrOwners: owners[start[l] + grid] is the rank of box `grid` of level l (nlev levels).  The workspace
// is the context's: hist[block][rank] -- the per-block counts of launch_tracer_migrate_count, turned into exclusive prefixes over
// the blocks by its scan launch -- which launch_tracer_migrate_pack reads for the same n and nranks.
#define CAD_TRACER_MAX_RANKS CASTRO_AMD_TRACER_MAX_RANKS
struct TrOwners { int nlev; int start[CAD_TRACER_MAX_LEVELS + 1]; };
struct TrMigrateWorkspace { int* hist = nullptr; size_t ints = 0; long long n = -1; int nranks = 0; };
int launch_tracer_migrate_count(const int* owners, int nown, const TrOwners& O, int nranks, int myrank, const castro_amd_tracers& T,
                                int* d_dest, int* d_counts, TrMigrateWorkspace* ws, TableCache* tables, hipStream_t stream,
                                Profiler* prof);
int launch_tracer_migrate_pack(int nranks, int myrank, const castro_amd_tracers& T, const int* d_dest, const castro_amd_tracers& out, long long* d_wire, long long nwire, TrMigrateWorkspace* ws,
                               hipStream_t stream, Profiler* prof);
int launch_tracer_unpack(const long long* d_wire, long long nrecv, const castro_amd_tracers& out, long long at, hipStream_t stream,
                         Profiler* prof);
// the gravity sources with a per-zone vector: GO / GN are 3-component FABs with one ghost zone around [lo, hi] (type 4)
int launch_old_grav_source_gfab(const DFab& U, const DFab& SRC, const int lo[3], const int hi[3], const DFab& GO,
                                int type, double dt, hipStream_t stream, Profiler* prof);
int launch_new_grav_source_gfab(const DFab& UO, const DFab& UN, const DFab& SRC, const DFab M[3], const int lo[3], const int hi[3],
                                const DFab& GO, const DFab& GN, int type, double dt, const double dx[3], hipStream_t stream,
                                Profiler* prof);
int launch_saxpy(const DFab& D, const DFab& S, const int lo[3], const int hi[3], double a, int ncomp,
                 hipStream_t stream, Profiler* prof);
int launch_fab_ops(int nops, const DFab* D, const DFab* X, const DFab* Y, const int* lo, const int* hi, const int* kind,
                   const int* dir, const int* side, const int* ncomp, const double* a, const double* b, hipStream_t stream, Profiler* prof,
                   const DevParams* P = nullptr, StagedTable* arena = nullptr);
int launch_apply_source(const DFab& D, const DFab& B, const DFab& S, const int lo[3], const int hi[3], double a, int nsrc,
                        const DevParams& P, int ntimes, hipStream_t stream, Profiler* prof);
int launch_cc_interp(const DFab& C, const DFab& F, const int lo[3], const int hi[3], int ncomp, hipStream_t stream, Profiler* prof);
int launch_fillpatch_shell(const DFab& C, const DFab& F, const int vlo[3], const int vhi[3], int ng, const DevParams& P, int ntimes,
                           hipStream_t stream, Profiler* prof);
int launch_avgdown(const DFab& F, const DFab& C, const int lo[3], const int hi[3], int ncomp, hipStream_t stream, Profiler* prof);
int launch_fluxreg_to_flux(const DFab& F, const DFab& R, const DFab& M, const int lo[3], const int hi[3], int ncomp,
                           hipStream_t stream, Profiler* prof);
int launch_fluxreg(const DFab& R, const DFab& X, const int lo[3], const int hi[3], int dir, int ncomp, double mult, int mode,
                   hipStream_t stream, Profiler* prof);
int launch_reflux(const DFab& U, const DFab& R, const int lo[3], const int hi[3], int dir, int side, int ncomp, double vol,
                  hipStream_t stream, Profiler* prof);
int launch_error_tag(const DFab& Q, int comp, const DFab& T, const int lo[3], const int hi[3], int kind, double value,
                     hipStream_t stream, Profiler* prof);
int launch_lincomb(const DFab& D, const DFab& X, const DFab& Y, const int lo[3], const int hi[3], double a, double bb, int ncomp,
                   hipStream_t stream, Profiler* prof);
int launch_derive(int which, const DFab& U, const DFab& D, int dcomp, const int lo[3], const int hi[3],
                  const double dx[3], const double problo[3], const DevParams& P, const double center[3],
                  hipStream_t stream, Profiler* prof);
int launch_bc_fill(const DFab& U, const int flo[3], const int fhi[3], int ncomp, const DevGeom& g,
                   const int lo_bc[3], const int hi_bc[3], hipStream_t stream, Profiler* prof);
// A box minus a box inside it as six slabs (z slabs over the full x-y extent, then y, then x): slab r holds the threads
// [start[r], start[r + 1]) of a launch, nn[r] zones from lo[r]
struct Slabs { int lo[6][3], nn[6][3]; long start[7]; };
// [flo, fhi] minus [blo, bhi]; flo <= blo <= bhi <= fhi in every direction
inline Slabs shell_slabs(const int flo[3], const int fhi[3], const int blo[3], const int bhi[3])
{
    const int lo[6][3] = { { flo[0], flo[1], flo[2] }, { flo[0], flo[1], bhi[2] + 1 }, { flo[0], flo[1], blo[2] },
                           { flo[0], bhi[1] + 1, blo[2] }, { flo[0], blo[1], blo[2] }, { bhi[0] + 1, blo[1], blo[2] } };
    const int hi[6][3] = { { fhi[0], fhi[1], blo[2] - 1 }, { fhi[0], fhi[1], fhi[2] }, { fhi[0], blo[1] - 1, bhi[2] },
                           { fhi[0], fhi[1], bhi[2] }, { blo[0] - 1, bhi[1], bhi[2] }, { fhi[0], bhi[1], bhi[2] } };
    Slabs S;
    S.start[0] = 0;
    for (int r = 0; r < 6; ++r) {
        long n = 1;
        for (int d = 0; d < 3; ++d) { S.lo[r][d] = lo[r][d]; S.nn[r][d] = hi[r][d] - lo[r][d] + 1; n *= S.nn[r][d] > 0 ? S.nn[r][d] : 0; }
        S.start[r + 1] = S.start[r] + n;
    }
    return S;
}
// the multipole boundary potential on the zones of [flo, fhi] outside the domain (poisson_kernels.hip)
int launch_multipole_phi_bc(const DFab& F, const int flo[3], const int fhi[3], const MpGeom& G, const double* d_q, hipStream_t stream,
                            Profiler* prof);
// the one-zone shell of the fine box [flo, fhi] of F from the coarse potentials O / N of the level below at weight a (k_phi_cf_bc)
int launch_phi_cf_bc(const DFab& F, const int flo[3], const int fhi[3], const DFab& O, const DFab& N, double a, hipStream_t stream,
                     Profiler* prof);
// the second half of the physical-boundary fill of a state FAB (extbc_kernels.hip): ambient_fill, then hse_fill
int launch_ext_bc_fill(const DFab& U, const int flo[3], const int fhi[3], const ::castro_amd_geom* geom, const DevParams& P,
                       const ::castro_amd_ext_bc* ext, int* d_unconverged, hipStream_t stream, Profiler* prof);
int launch_copy(const DFab& dst, const DFab& src, const int lo[3], const int hi[3], int ncomp,
                hipStream_t stream, Profiler* prof);
int launch_pack(const DFab& f, const int lo[3], const int hi[3], int ncomp, double* buf, int unpack,
                hipStream_t stream, Profiler* prof);
int launch_pack_regions(const DFab& f, int nreg, const int* lo, const int* hi, const long long* off, int ncomp, double* buf,
                        int unpack, hipStream_t stream, Profiler* prof);
int launch_sedov_init(const DFab& U, const int lo[3], const int hi[3], const DevParams& P,
                      const double dx[3], const double problo[3], const double center[3],
                      double r_init, double e_exp, double e_ambient, double temp_ambient,
                      double dens_ambient, int nsub, hipStream_t stream, Profiler* prof);
int launch_sod_init(const DFab& U, const int lo[3], const int hi[3], const double dx[3],
                    const double problo[3], double split, int idir0,
                    double rho_l, double u_l, double rhoe_l, double T_l,
                    double rho_r, double u_r, double rhoe_r, double T_r,
                    hipStream_t stream, Profiler* prof);

} // namespace cad

// capi.hip -- the C ABI (include/castro_hydro_amd.h) over the HIP kernels.
// Plain pointers and sizes only; no torch, no AMReX.  One context per (device, stream).
#include <hip/hip_runtime.h>
#include <vector>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include "../../include/castro_hydro_amd.h"
#include <cstdlib>
#include <cstdint>
#include "ctu_kernels.h"

using namespace cad;

struct castro_amd_ctx {
    int device = 0;
    LaunchKnobs knobs;         // read from the environment at creation, never written again
    double* arena = nullptr;
    size_t arena_doubles = 0;
    int* d_status = nullptr;
    int* h_status = nullptr;   // pinned
    castro_amd_fab src_corr = { nullptr, { 0, 0, 0 }, { 0, 0, 0 }, 0 };     // Castro::source_corrector
    Profiler prof;
    // a second stream for launches that depend on nothing the main stream is about to produce (k_divu beside the trace
    // kernel), forked from and joined to the caller's stream with events inside one call: CASTRO_AMD_SIDE_STREAM=0 turns it off
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // device tables (dev_table.h), one per launch family: a source call with diffusion has two of them in flight
    StagedTable ops_arena;                          // castro_amd_fab_ops_p calls with more than 16 operations, castro_amd_sources_mf*
    StagedTable level_arena;                        // a level-wide hydro launch (castro_amd_ctu_hydro_mf)
    StagedTable diff_arena;                         // a thermal-diffusion launch (castro_amd_temp_diffusion_*)
    hipEvent_t mf_fork = nullptr, mf_join = nullptr;   // castro_amd_ctu_hydro_mf: fork from / join to the caller's stream
    StagedTable diag_arena;                         // castro_amd_integrated_quantities_mf
    DiagWorkspace diag_ws;                          // its rows of partial sums, one per workgroup
    MonoWorkspace mono_ws;                          // castro_amd_radial_mass_mf: rows, counts and device box tables
    TableCache pm_tables{32};                       // castro_amd_add_pointmass_mf / castro_amd_pointmass_*_mf
    TableCache tr_tables{32};                       // castro_amd_tracer_*
    TrMigrateWorkspace tr_migrate;                  // castro_amd_tracer_migrate_count -> _pack: per-block counts per rank
    StagedTable pack_arena;                         // castro_amd_fab_pack / castro_amd_fab_unpack
    DiagWorkspace pack_ws;                          // castro_amd_fab_pack: one (min, max) pair per workgroup
    StagedTable mp_arena;                           // castro_amd_multipole_moments_mf
    DiagWorkspace mp_ws;                            // its rows of partial sums, one per workgroup and order m
};

namespace cad {

// ---- profiler -------------------------------------------------------------------------
static hipEvent_t prof_event(Profiler* p)
{
    if (!p->pool.empty()) { hipEvent_t e = p->pool.back(); p->pool.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

void prof_begin(Profiler* p, const char* name, hipStream_t s)
{
    if (!p || !p->enabled) return;
    int idx = -1;
    for (size_t n = 0; n < p->recs.size(); ++n) if (p->recs[n].name == name) { idx = (int)n; break; }
    if (idx < 0) { p->recs.push_back(Profiler::Rec()); p->recs.back().name = name; idx = (int)p->recs.size() - 1; }
    p->cur = idx;
    p->cur_e0 = prof_event(p);
    p->cur_e1 = prof_event(p);
    hipEventRecord(p->cur_e0, s);
}

void prof_end(Profiler* p, hipStream_t s)
{
    if (!p || !p->enabled || p->cur < 0) return;
    hipEventRecord(p->cur_e1, s);
    p->pending.push_back({ p->cur, p->cur_e0, p->cur_e1 });
    p->cur = -1;
}

void prof_collect(Profiler* p)
{
    for (auto& pe : p->pending) {
        hipEventSynchronize(pe.e1);
        float ms = 0.f;
        hipEventElapsedTime(&ms, pe.e0, pe.e1);
        p->recs[pe.rec].total_ms += ms;
        p->recs[pe.rec].launches += 1;
        p->pool.push_back(pe.e0);
        p->pool.push_back(pe.e1);
    }
    p->pending.clear();
}

} // namespace cad

// ---- helpers ------------------------------------------------------------------------------
static DFab to_dfab(const castro_amd_fab* f)
{
    DFab d;
    if (!f || !f->p) { d.p = nullptr; d.lo[0] = d.lo[1] = d.lo[2] = 0; d.sy = d.sz = d.sn = 0; return d; }
    d.p = f->p;
    long nx = f->hi[0] - f->lo[0] + 1, ny = f->hi[1] - f->lo[1] + 1, nz = f->hi[2] - f->lo[2] + 1;
    for (int n = 0; n < 3; ++n) d.lo[n] = f->lo[n];
    d.sy = nx; d.sz = nx * ny; d.sn = nx * ny * nz;
    return d;
}

static bool fab_contains(const castro_amd_fab* f, const int lo[3], const int hi[3])
{
    for (int d = 0; d < 3; ++d) if (f->lo[d] > lo[d] || f->hi[d] < hi[d]) return false;
    return true;
}

static DevParams to_devparams(const castro_amd_params* p)
{
    DevParams P;
    P.gamma = p->eos_gamma;
    P.small_dens = p->small_dens; P.small_pres = p->small_pres;
    P.small_temp = p->small_temp; P.small_ener = p->small_ener;
    P.small_dens_ener = p->small_dens * p->small_ener;
    P.difmag = p->difmag;
    P.cg_tol = p->cg_tol;
    P.eta1 = p->dual_energy_eta1; P.eta2 = p->dual_energy_eta2;
    P.small_x = p->small_x;
    P.abar = p->abar;
    P.riemann_solver = p->riemann_solver; P.use_flattening = p->use_flattening;
    P.first_order_hydro = p->first_order_hydro; P.hybrid_riemann = p->hybrid_riemann;
    P.cg_maxiter = p->cg_maxiter; P.cg_blend = p->cg_blend;
    P.reset_density = p->transverse_reset_density; P.reset_rhoe = p->transverse_reset_rhoe;
    P.use_eos = p->transverse_use_eos;
    P.ppm_temp_fix = p->ppm_temp_fix;
    P.ppm_type = p->ppm_type; P.plm_iorder = p->plm_iorder; P.plm_limiter = p->plm_limiter; P.use_pslope = p->use_pslope;
    P.pslope_cutoff_density = p->pslope_cutoff_density;
    P.cfl = p->cfl; P.speed_limit = p->speed_limit;
    P.limit_small_dens = p->limit_fluxes_on_small_dens; P.limit_large_vel = p->limit_fluxes_on_large_vel;
    P.source_term_predictor = p->source_term_predictor;
    P.dtp = nullptr;
    return P;
}

namespace cad { DevParams unit_devparams(const castro_amd_params* p) { return to_devparams(p); } }

static DevGeom to_devgeom(const castro_amd_geom* g)
{
    DevGeom G;
    for (int d = 0; d < 3; ++d) {
        G.dx[d] = g->dx[d];
        G.domlo[d] = g->domlo[d]; G.domhi[d] = g->domhi[d];
        G.wall_lo[d] = (g->lo_bc[d] >= 3) ? 1 : 0;
        G.wall_hi[d] = (g->hi_bc[d] >= 3) ? 1 : 0;
        G.sym_lo[d] = (g->lo_bc[d] == 3) ? 1 : 0;
        G.sym_hi[d] = (g->hi_bc[d] == 3) ? 1 : 0;
    }
    return G;
}

// x extent of a scratch plane: the tile grown by 4, preceded by xpad unused columns (the context's LaunchKnobs::xpad) and rounded
// up to a multiple of 16 doubles when xpad > 0, so that zone lo[0] - 4 + (4 + xpad) starts a 128-byte line in every row
static int scratch_nx(int xpad, int nx) { return xpad > 0 ? ((nx + 8 + xpad + 15) & ~15) : nx + 8; }

static size_t plane_doubles(int xpad, int nx, int ny, int nz)
{
    size_t n = (size_t)scratch_nx(xpad, nx) * (ny + 8) * (nz + 8);
    return (n + 31) & ~(size_t)31;     // keep every component plane 256-byte aligned
}

// number of component planes in the scratch arena
static constexpr int kPlanes = NPRIM + 2 + 6 + 6 * NEDGE + 3 * NF1 + 6 * NF1 + 3 * NFIN;
static constexpr int kPlanesResetRhoe = 9;     // F1E[3] + F2E[6], only with transverse_reset_rhoe = 1

extern "C" {

#ifdef CAD_NUMERICS_CONTRACT
#define CAD_NUMERICS_NAME "contract"
#else
#define CAD_NUMERICS_NAME "exact"
#endif
const char* castro_amd_version(void) { return "castro_hydro_amd " CASTRO_AMD_RELEASE " (gfx950, numerics=" CAD_NUMERICS_NAME ")"; }
int castro_amd_abi_version(void) { return CASTRO_AMD_ABI_VERSION; }
const char* castro_amd_numerics(void) { return CAD_NUMERICS_NAME; }

// Source/driver/_cpp_parameters defaults + Exec/hydro_tests/Sedov/inputs.3d.sph(.testsuite)
void castro_amd_default_params(castro_amd_params* p)
{
    std::memset(p, 0, sizeof(*p));
    p->ppm_type = 1; p->riemann_solver = 0; p->use_flattening = 1; p->hybrid_riemann = 0;
    p->first_order_hydro = 0; p->cg_maxiter = 12; p->cg_blend = 2;
    p->transverse_use_eos = 0; p->transverse_reset_density = 1; p->transverse_reset_rhoe = 0;
    p->ppm_temp_fix = 0;
    p->plm_iorder = 2; p->plm_limiter = 2; p->use_pslope = 1; p->pslope_cutoff_density = -1.e20;
    p->limit_fluxes_on_small_dens = 0; p->limit_fluxes_on_large_vel = 0; p->speed_limit = 0.0;
    p->source_term_predictor = 0;
    p->difmag = 0.1;
    p->small_dens = -1.e200; p->small_temp = -1.e200; p->small_pres = -1.e200; p->small_ener = -1.e200;
    p->cg_tol = 1.0e-5;
    p->dual_energy_eta1 = 1.0; p->dual_energy_eta2 = 1.0e-4;
    p->cfl = 0.5; p->init_shrink = 0.01; p->change_max = 1.1;
    p->eos_gamma = 1.4; p->small_x = 1.e-30; p->T_guess = 1.e8; p->abar = 1.0;
    castro_amd_finalize_params(p);
}

// Castro_setup.cpp:222-236 and :259-288
void castro_amd_finalize_params(castro_amd_params* p)
{
    if (p->small_dens < 0.0) p->small_dens = 1.e-100;
    if (p->small_temp < 0.0) p->small_temp = 1.e-100;
    if (p->small_pres < 0.0) p->small_pres = 1.e-100;
    if (p->small_ener < 0.0) p->small_ener = 1.e-100;
    // eos(eos_input_rt) at (small_dens, small_temp)
    // xn = 1 / NumSpec (Castro_setup.cpp:279): mu = abar = 1 / sum_k(xn_k / A_k)
    const double mu = 1.0 / (1.0 * (1.0 / p->abar));
    double e = K_B * p->small_temp / ((p->eos_gamma - 1.0) * (mu * M_U));
    double pr = (p->eos_gamma - 1.0) * p->small_dens * e;
    if (p->small_pres < pr) p->small_pres = pr;
    if (p->small_ener < e) p->small_ener = e;
}

int castro_amd_ctx_create(castro_amd_ctx** out, int device)
{
    if (!out) return CASTRO_AMD_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        std::fprintf(stderr, "castro_hydro_amd: no HIP device available -- this library has no CPU fallback\n");
        return CASTRO_AMD_ERR_HIP;
    }
    if (device < 0 || device >= ndev) return CASTRO_AMD_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return CASTRO_AMD_ERR_HIP;
    castro_amd_ctx* c = new (std::nothrow) castro_amd_ctx();
    if (!c) return CASTRO_AMD_ERR_NOMEM;
    c->device = device;
    if (hipMalloc(&c->d_status, sizeof(int)) != hipSuccess) { delete c; return CASTRO_AMD_ERR_NOMEM; }
    hipMemset(c->d_status, 0, sizeof(int));
    if (hipHostMalloc(&c->h_status, sizeof(int)) != hipSuccess) { hipFree(c->d_status); delete c; return CASTRO_AMD_ERR_NOMEM; }
    // a variable that is not set gives its default; what is read here holds for this context, whatever is created after it
    c->knobs = launch_knobs_from_env();
    if (c->knobs.side_stream) {
        if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
            castro_amd_ctx_destroy(c);
            return CASTRO_AMD_ERR_HIP;
        }
    }
    *out = c;
    return CASTRO_AMD_OK;
}

void castro_amd_ctx_destroy(castro_amd_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->side) { hipStreamSynchronize(c->side); hipStreamDestroy(c->side); }
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    if (c->mf_fork) hipEventDestroy(c->mf_fork);
    if (c->mf_join) hipEventDestroy(c->mf_join);
    for (StagedTable* t : { &c->ops_arena, &c->level_arena, &c->diff_arena, &c->diag_arena, &c->pack_arena, &c->mp_arena }) t->release();
    if (c->diag_ws.p) hipFree(c->diag_ws.p);
    if (c->mp_ws.p) hipFree(c->mp_ws.p);
    if (c->pack_ws.p) hipFree(c->pack_ws.p);
    mono_workspace_free(&c->mono_ws);
    c->pm_tables.release();
    c->tr_tables.release();
    if (c->tr_migrate.hist) hipFree(c->tr_migrate.hist);
    prof_collect(&c->prof);
    for (auto e : c->prof.pool) hipEventDestroy(e);
    if (c->arena) hipFree(c->arena);
    if (c->d_status) hipFree(c->d_status);
    if (c->h_status) hipHostFree(c->h_status);
    delete c;
}

static int reserve_planes(castro_amd_ctx* c, int nx, int ny, int nz, int planes)
{
    if (!c || nx <= 0 || ny <= 0 || nz <= 0) return CASTRO_AMD_ERR_ARG;
    size_t need = plane_doubles(c->knobs.xpad, nx, ny, nz) * (size_t)planes;
    if (need <= c->arena_doubles) return CASTRO_AMD_OK;
    hipSetDevice(c->device);
    if (c->arena) { hipDeviceSynchronize(); hipFree(c->arena); c->arena = nullptr; c->arena_doubles = 0; }
    if (hipMalloc(&c->arena, need * sizeof(double)) != hipSuccess) return CASTRO_AMD_ERR_NOMEM;
    c->arena_doubles = need;
    return CASTRO_AMD_OK;
}

int castro_amd_ctx_reserve(castro_amd_ctx* c, int nx, int ny, int nz)
{
    return reserve_planes(c, nx, ny, nz, kPlanes);
}

long long castro_amd_ctx_scratch_bytes(const castro_amd_ctx* c)
{
    return c ? (long long)(c->arena_doubles * sizeof(double)) : 0;
}

int castro_amd_ctx_status(castro_amd_ctx* c, void* stream)
{
    if (!c) return CASTRO_AMD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipMemcpyAsync(c->h_status, c->d_status, sizeof(int), hipMemcpyDeviceToHost, s);
    hipMemsetAsync(c->d_status, 0, sizeof(int), s);
    if (hipStreamSynchronize(s) != hipSuccess) return CASTRO_AMD_ERR_HIP;
    return *c->h_status;
}

int castro_amd_ctu_hydro_fab(castro_amd_ctx* c, const int bxlo[3], const int bxhi[3],
                             const int vbxlo[3], const int vbxhi[3],
                             const castro_amd_fab* Sborder, const castro_amd_fab* src,
                             const castro_amd_fab* S_new, const castro_amd_fab flux_out[3],
                             const castro_amd_fab mass_flux_out[3], const castro_amd_fab qe_out[3],
                             const castro_amd_geom* geom, const castro_amd_params* params,
                             double time, double dt, int flags, void* stream)
{
    return castro_amd_ctu_hydro_clean_fab(c, bxlo, bxhi, vbxlo, vbxhi, Sborder, src, S_new, flux_out, mass_flux_out, qe_out,
                                          geom, params, time, dt, flags, 0, nullptr, stream);
}

int castro_amd_ctu_hydro_clean_fab(castro_amd_ctx* c, const int bxlo[3], const int bxhi[3],
                                   const int vbxlo[3], const int vbxhi[3],
                                   const castro_amd_fab* Sborder, const castro_amd_fab* src,
                                   const castro_amd_fab* S_new, const castro_amd_fab flux_out[3],
                                   const castro_amd_fab mass_flux_out[3], const castro_amd_fab qe_out[3],
                                   const castro_amd_geom* geom, const castro_amd_params* params,
                                   double time, double dt, int flags, int clean_ntimes, double* d_out, void* stream)
{
    castro_amd_hydro_opts o;
    o.flags = flags; o.clean_ntimes = clean_ntimes; o.d_out = d_out; o.sborder_clean_ntimes = 0; o.d_dt = nullptr;
    return castro_amd_ctu_hydro_fab_ex(c, bxlo, bxhi, vbxlo, vbxhi, Sborder, src, S_new, flux_out, mass_flux_out, qe_out,
                                       geom, params, time, dt, &o, stream);
}

// One box of a hydro call, checked and translated: what castro_amd_ctu_hydro_fab_ex and the level-wide launch of
// castro_amd_ctu_hydro_mf have in common.
struct PreparedBox {
    Tile t;
    DFab dS, dN, dSrc, dF[3], dM[3], dQ[3], dCorr;
    int acc_hi[3];
    int nx, ny, nz;
    bool reset_rhoe;
};

static int prepare_box(castro_amd_ctx* c, const int bxlo[3], const int bxhi[3], const int vbxlo[3], const int vbxhi[3],
                       const castro_amd_fab* Sborder, const castro_amd_fab* src, const castro_amd_fab* S_new,
                       const castro_amd_fab flux_out[3], const castro_amd_fab mass_flux_out[3], const castro_amd_fab qe_out[3],
                       const castro_amd_geom* geom, const castro_amd_params* params, const castro_amd_hydro_opts* opts, PreparedBox& B)
{
    if (!opts) return CASTRO_AMD_ERR_ARG;
    const int flags = opts->flags, clean_ntimes = opts->clean_ntimes, sb_clean = opts->sborder_clean_ntimes;
    if (clean_ntimes < 0 || sb_clean < 0) return CASTRO_AMD_ERR_ARG;
    const int light = flags & (CASTRO_AMD_STAGE_VALID | CASTRO_AMD_STAGE_REST);
    if (light == (CASTRO_AMD_STAGE_VALID | CASTRO_AMD_STAGE_REST)) return CASTRO_AMD_ERR_ARG;
    if ((light || (flags & CASTRO_AMD_BC_FILL)) && (flags & (CASTRO_AMD_STAGE_A | CASTRO_AMD_STAGE_B))) return CASTRO_AMD_ERR_ARG;
    if (sb_clean > 0 || light || (flags & CASTRO_AMD_BC_FILL)) {
        // in-place cleaning of Sborder, the valid / rest split and the fused boundary fill: whole-box calls only, never with the
        // round-2 staging (see the header)
        if (sb_clean > 0 && (flags & (CASTRO_AMD_STAGE_A | CASTRO_AMD_STAGE_B))) return CASTRO_AMD_ERR_ARG;
        if (vbxlo && vbxhi)
            for (int d = 0; d < 3; ++d) if (vbxlo[d] != bxlo[d] || vbxhi[d] != bxhi[d]) return CASTRO_AMD_ERR_ARG;
        // cleaned valid zones + a separate k_bc_fill + cleaning the shell would clean the boundary zones twice over
        if (sb_clean > 0 && (flags & CASTRO_AMD_STAGE_REST) && !(flags & CASTRO_AMD_BC_FILL)) return CASTRO_AMD_ERR_ARG;
    }
    if (!c || !bxlo || !bxhi || !Sborder || !Sborder->p || !S_new || !S_new->p || !geom || !params)
        return CASTRO_AMD_ERR_ARG;
    if (Sborder->ncomp != NUM_STATE || S_new->ncomp != NUM_STATE) return CASTRO_AMD_ERR_ARG;
    if (geom->coord != 0) return CASTRO_AMD_ERR_UNSUPPORTED;
    if (params->ppm_type != 0 && params->ppm_type != 1) return CASTRO_AMD_ERR_ARG;
    if (params->riemann_solver < 0 || params->riemann_solver > 2) return CASTRO_AMD_ERR_ARG;
    if (params->hybrid_riemann != 0 && params->hybrid_riemann != 1) return CASTRO_AMD_ERR_ARG;
    if (params->ppm_temp_fix < 0 || params->ppm_temp_fix > 2) return CASTRO_AMD_ERR_ARG;    // 1 is a no-op in the CTU path

    Tile& t = B.t;
    int glo[3], ghi[3];
    for (int d = 0; d < 3; ++d) {
        if (bxhi[d] < bxlo[d]) return CASTRO_AMD_ERR_ARG;
        t.lo[d] = bxlo[d]; t.hi[d] = bxhi[d];
        t.glo[d] = glo[d] = bxlo[d] - CASTRO_AMD_NUM_GROW;
        ghi[d] = bxhi[d] + CASTRO_AMD_NUM_GROW;
    }
    const int nx = bxhi[0] - bxlo[0] + 1, ny = bxhi[1] - bxlo[1] + 1, nz = bxhi[2] - bxlo[2] + 1;
    B.nx = nx; B.ny = ny; B.nz = nz;
    t.glo[0] -= c->knobs.xpad;
    t.NX = scratch_nx(c->knobs.xpad, nx); t.NY = ny + 8; t.NZ = nz + 8;
    t.NC = (long)plane_doubles(c->knobs.xpad, nx, ny, nz);

    if (!fab_contains(Sborder, glo, ghi)) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(S_new, bxlo, bxhi)) return CASTRO_AMD_ERR_ARG;
    // the kernels address a component plane with a 32-bit byte offset: scratch planes and the caller's component
    // planes must stay below 4 GiB (a box of more than ~800^3 zones has to be tiled by the caller)
    {
        const double lim = 4294967296.0;
        auto plane_bytes = [](const castro_amd_fab* f) {
            return 8.0 * (double)(f->hi[0] - f->lo[0] + 1) * (double)(f->hi[1] - f->lo[1] + 1) * (double)(f->hi[2] - f->lo[2] + 1);
        };
        if (8.0 * (double)t.NC >= lim || plane_bytes(Sborder) >= lim || plane_bytes(S_new) >= lim) return CASTRO_AMD_ERR_UNSUPPORTED;
        for (int d = 0; d < 3; ++d) {
            if (flux_out && flux_out[d].p && plane_bytes(&flux_out[d]) >= lim) return CASTRO_AMD_ERR_UNSUPPORTED;
            if (mass_flux_out && mass_flux_out[d].p && plane_bytes(&mass_flux_out[d]) >= lim) return CASTRO_AMD_ERR_UNSUPPORTED;
            if (qe_out && qe_out[d].p && plane_bytes(&qe_out[d]) >= lim) return CASTRO_AMD_ERR_UNSUPPORTED;
        }
    }
    if (src && src->p) {
        // old_source: NSRC = 7 components, NUM_GROW_SRC = 3 ghost zones (Castro_setup.cpp:317-327)
        int s3lo[3], s3hi[3];
        for (int d = 0; d < 3; ++d) { s3lo[d] = bxlo[d] - 3; s3hi[d] = bxhi[d] + 3; }
        if (src->ncomp < 6 || !fab_contains(src, s3lo, s3hi)) return CASTRO_AMD_ERR_ARG;
    }
    B.reset_rhoe = params->transverse_reset_rhoe == 1;
    B.dS = to_dfab(Sborder); B.dN = to_dfab(S_new); B.dSrc = to_dfab(src);
    for (int d = 0; d < 3; ++d) {
        int flo[3] = { bxlo[0], bxlo[1], bxlo[2] }, fhi[3] = { bxhi[0], bxhi[1], bxhi[2] };
        fhi[d] += 1;
        // mfi.nodaltilebox(d): the high face belongs to this tile only at the valid box's high end
        B.acc_hi[d] = bxhi[d] + 1;
        if (vbxhi && B.acc_hi[d] <= vbxhi[d]) B.acc_hi[d] -= 1;
        fhi[d] = B.acc_hi[d];
        const castro_amd_fab* f = flux_out ? &flux_out[d] : nullptr;
        const castro_amd_fab* m = mass_flux_out ? &mass_flux_out[d] : nullptr;
        const castro_amd_fab* q = qe_out ? &qe_out[d] : nullptr;
        if (f && f->p && (f->ncomp != NUM_STATE || !fab_contains(f, flo, fhi))) return CASTRO_AMD_ERR_ARG;
        if (m && m->p && (m->ncomp != 1 || !fab_contains(m, flo, fhi))) return CASTRO_AMD_ERR_ARG;
        if (q && q->p && (q->ncomp != NGDNV || !fab_contains(q, flo, fhi))) return CASTRO_AMD_ERR_ARG;
        B.dF[d] = to_dfab(f); B.dM[d] = to_dfab(m); B.dQ[d] = to_dfab(q);
    }
    B.dCorr = to_dfab(nullptr);
    // the reference always has source_corrector defined when the predictor is on (Castro_advance_ctu.cpp:60-62):
    // running without it would silently drop the predictor
    if (params->source_term_predictor == 1 && src && src->p && !c->src_corr.p) return CASTRO_AMD_ERR_ARG;
    if (params->source_term_predictor == 1 && c->src_corr.p && src && src->p) {
        int s3lo[3], s3hi[3];
        for (int d = 0; d < 3; ++d) { s3lo[d] = bxlo[d] - 3; s3hi[d] = bxhi[d] + 3; }
        if (!fab_contains(&c->src_corr, s3lo, s3hi)) return CASTRO_AMD_ERR_ARG;
        B.dCorr = to_dfab(&c->src_corr);
    }
    return CASTRO_AMD_OK;
}

// the scratch arrays of one box, carved from p; returns the first double behind them
static double* carve_scratch(double* p, const Tile& t, bool reset_rhoe, DevScratch& S)
{
    const size_t NC = (size_t)t.NC;
    S.Q = p; p += NC * NPRIM;
    S.DIV = p; p += NC;
    S.SHK = p; p += NC;
    S.SRCQ = p; p += NC * 6;
    for (int d = 0; d < 3; ++d) { S.QM[d] = p; p += NC * NEDGE; S.QP[d] = p; p += NC * NEDGE; }
    for (int d = 0; d < 3; ++d) { S.F1[d] = p; p += NC * NF1; }
    for (int d = 0; d < 6; ++d) { S.F2[d] = p; p += NC * NF1; }
    for (int d = 0; d < 3; ++d) { S.FL[d] = p; p += NC * NFIN; }
    for (int d = 0; d < 3; ++d) { S.F1E[d] = reset_rhoe ? p : nullptr; if (reset_rhoe) p += NC; }
    for (int d = 0; d < 6; ++d) { S.F2E[d] = reset_rhoe ? p : nullptr; if (reset_rhoe) p += NC; }
    return p;
}

int castro_amd_ctu_hydro_fab_ex(castro_amd_ctx* c, const int bxlo[3], const int bxhi[3],
                                const int vbxlo[3], const int vbxhi[3],
                                const castro_amd_fab* Sborder, const castro_amd_fab* src,
                                const castro_amd_fab* S_new, const castro_amd_fab flux_out[3],
                                const castro_amd_fab mass_flux_out[3], const castro_amd_fab qe_out[3],
                                const castro_amd_geom* geom, const castro_amd_params* params,
                                double time, double dt, const castro_amd_hydro_opts* opts, void* stream)
{
    (void)time;
    PreparedBox B;
    int rc = prepare_box(c, bxlo, bxhi, vbxlo, vbxhi, Sborder, src, S_new, flux_out, mass_flux_out, qe_out, geom, params, opts, B);
    if (rc != CASTRO_AMD_OK) return rc;
    hipSetDevice(c->device);
    rc = reserve_planes(c, B.nx, B.ny, B.nz, kPlanes + (B.reset_rhoe ? kPlanesResetRhoe : 0));
    if (rc != CASTRO_AMD_OK) return rc;
    DevScratch S;
    carve_scratch(c->arena, B.t, B.reset_rhoe, S);
    LaunchAux aux;
    aux.knobs = c->knobs;
    aux.sb_clean = opts->sborder_clean_ntimes;
    aux.side = c->side; aux.ev_fork = c->ev_fork; aux.ev_join = c->ev_join;
    for (int d = 0; d < 3; ++d) { aux.bc_lo[d] = geom->lo_bc[d]; aux.bc_hi[d] = geom->hi_bc[d]; }
    DevParams devP = to_devparams(params);
    devP.dtp = opts->d_dt;
    return launch_ctu_hydro(B.t, S, B.dS, B.dSrc, B.dN, B.dF, B.dM, B.dQ, to_devgeom(geom), devP, dt, opts->flags,
                            B.acc_hi, c->d_status, (hipStream_t)stream, &c->prof, opts->clean_ntimes, opts->d_out, B.dCorr, aux);
}

int castro_amd_step_control(castro_amd_ctx* c, double* d_red, double* d_ctl, const castro_amd_params* params,
                            double max_dt, double fixed_dt, double stop_time, int use_retry, void* stream)
{
    if (!c || !d_red || !d_ctl || !params) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_step_control(d_red, d_ctl, params->cfl, params->change_max, params->small_dens, max_dt, fixed_dt, stop_time,
                               use_retry ? 1 : 0, (hipStream_t)stream, &c->prof);
}

int castro_amd_clean_state_fab(castro_amd_ctx* c, const castro_amd_fab* state, const int lo[3], const int hi[3],
                               const castro_amd_params* params, int ntimes, void* stream)
{
    if (!c || !state || !state->p || !params || state->ncomp != NUM_STATE || ntimes < 1) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_clean_state(to_dfab(state), lo, hi, to_devparams(params), ntimes, (hipStream_t)stream, &c->prof);
}

int castro_amd_clean_state_reduce_fab(castro_amd_ctx* c, const castro_amd_fab* state, const int lo[3], const int hi[3],
                                      const castro_amd_geom* geom, const castro_amd_params* params, int ntimes,
                                      double* d_out, void* stream)
{
    if (!c || !state || !state->p || !geom || !params || !d_out || state->ncomp != NUM_STATE || ntimes < 1)
        return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_clean_state_reduce(to_dfab(state), lo, hi, to_devgeom(geom), to_devparams(params), ntimes, d_out,
                                     (hipStream_t)stream, &c->prof);
}

int castro_amd_estdt_fab(castro_amd_ctx* c, const castro_amd_fab* state, const int lo[3], const int hi[3],
                         const castro_amd_geom* geom, const castro_amd_params* params, double* d_out, void* stream)
{
    if (!c || !state || !state->p || !geom || !params || !d_out || state->ncomp != NUM_STATE) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_estdt(to_dfab(state), lo, hi, to_devgeom(geom), to_devparams(params), d_out, (hipStream_t)stream, &c->prof);
}

int castro_amd_old_gravity_source_fab(castro_amd_ctx* c, const castro_amd_fab* state, const castro_amd_fab* source,
                                      const int lo[3], const int hi[3], const double grav[3], int grav_source_type,
                                      double dt, void* stream)
{
    if (!c || !state || !state->p || !source || !source->p || !grav) return CASTRO_AMD_ERR_ARG;
    if (state->ncomp != NUM_STATE || source->ncomp < 7 || grav_source_type < 1 || grav_source_type > 4) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state, lo, hi) || !fab_contains(source, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_old_grav_source(to_dfab(state), to_dfab(source), lo, hi, grav, grav_source_type, dt, (hipStream_t)stream, &c->prof);
}

// the three mass-flux FABs of [lo, hi]: one component each, on the faces of their direction
static bool mass_flux_dfabs(const castro_amd_fab mass_fluxes[3], const int lo[3], const int hi[3], DFab M[3])
{
    for (int d = 0; d < 3; ++d) {
        int fhi[3] = { hi[0], hi[1], hi[2] };
        fhi[d] += 1;
        if (!mass_fluxes[d].p || mass_fluxes[d].ncomp != 1 || !fab_contains(&mass_fluxes[d], lo, fhi)) return false;
        M[d] = to_dfab(&mass_fluxes[d]);
    }
    return true;
}

int castro_amd_new_gravity_source_fab(castro_amd_ctx* c, const castro_amd_fab* state_old, const castro_amd_fab* state_new,
                                      const castro_amd_fab* source, const castro_amd_fab mass_fluxes[3],
                                      const int lo[3], const int hi[3], const double grav[3], int grav_source_type,
                                      double dt, const castro_amd_geom* geom, void* stream)
{
    if (!c || !state_old || !state_old->p || !state_new || !state_new->p || !source || !source->p || !mass_fluxes || !grav || !geom)
        return CASTRO_AMD_ERR_ARG;
    if (state_old->ncomp != NUM_STATE || state_new->ncomp != NUM_STATE || source->ncomp < 7) return CASTRO_AMD_ERR_ARG;
    if (grav_source_type < 1 || grav_source_type > 4 || geom->coord != 0) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state_old, lo, hi) || !fab_contains(state_new, lo, hi) || !fab_contains(source, lo, hi)) return CASTRO_AMD_ERR_ARG;
    DFab M[3];
    if (!mass_flux_dfabs(mass_fluxes, lo, hi, M)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_new_grav_source(to_dfab(state_old), to_dfab(state_new), to_dfab(source), M, lo, hi, grav, grav_source_type,
                                  dt, geom->dx, (hipStream_t)stream, &c->prof);
}

int castro_amd_old_rotation_source_fab(castro_amd_ctx* c, const castro_amd_fab* state, const castro_amd_fab* source,
                                       const int lo[3], const int hi[3], const castro_amd_rotation* rot,
                                       const castro_amd_geom* geom, double dt, void* stream)
{
    if (!c || !state || !state->p || !source || !source->p || !rot || !geom) return CASTRO_AMD_ERR_ARG;
    if (state->ncomp != NUM_STATE || source->ncomp < 7 || rot->rot_source_type < 1 || rot->rot_source_type > 4 || geom->coord != 0)
        return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state, lo, hi) || !fab_contains(source, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_old_rot_source(to_dfab(state), to_dfab(source), lo, hi, rot, geom, dt, (hipStream_t)stream, &c->prof);
}

int castro_amd_new_rotation_source_fab(castro_amd_ctx* c, const castro_amd_fab* state_old, const castro_amd_fab* state_new,
                                       const castro_amd_fab* source, const castro_amd_fab mass_fluxes[3],
                                       const int lo[3], const int hi[3], const castro_amd_rotation* rot,
                                       const castro_amd_geom* geom, double dt, void* stream)
{
    if (!c || !state_old || !state_old->p || !state_new || !state_new->p || !source || !source->p || !mass_fluxes || !rot || !geom)
        return CASTRO_AMD_ERR_ARG;
    if (state_old->ncomp != NUM_STATE || state_new->ncomp != NUM_STATE || source->ncomp < 7) return CASTRO_AMD_ERR_ARG;
    if (rot->rot_source_type < 1 || rot->rot_source_type > 4 || geom->coord != 0 || !(dt > 0.0)) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state_old, lo, hi) || !fab_contains(state_new, lo, hi) || !fab_contains(source, lo, hi)) return CASTRO_AMD_ERR_ARG;
    DFab M[3];
    if (!mass_flux_dfabs(mass_fluxes, lo, hi, M)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_new_rot_source(to_dfab(state_old), to_dfab(state_new), to_dfab(source), M, lo, hi, rot, geom, dt,
                                 (hipStream_t)stream, &c->prof);
}

int castro_amd_new_sponge_source_fab(castro_amd_ctx* c, const castro_amd_fab* state_new, const castro_amd_fab* source,
                                     const int lo[3], const int hi[3], const castro_amd_sponge* sponge,
                                     const castro_amd_geom* geom, const castro_amd_params* params, double dt, void* stream)
{
    if (!c || !state_new || !state_new->p || !source || !source->p || !lo || !hi || !sponge || !geom || !params) return CASTRO_AMD_ERR_ARG;
    if (state_new->ncomp != NUM_STATE || source->ncomp < 7) return CASTRO_AMD_ERR_ARG;
    if (geom->coord != 0 || !(dt > 0.0) || !(sponge->timescale > 0.0)) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state_new, lo, hi) || !fab_contains(source, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_new_sponge_source(to_dfab(state_new), to_dfab(source), lo, hi, sponge, geom, to_devparams(params), dt,
                                    (hipStream_t)stream, &c->prof);
}

// ---- the source stages and the level reductions for every box of a level in one call (include/castro_hydro_amd.h) ----
// ---- thermal diffusion (diffusion_kernels.hip) ----
// the operator's boundary conditions (Diffusion.cpp:99-126): Neumann, except Dirichlet for Inflow on a low face and for Symmetry
// on a high face -- those two need AMReX's high-order extrapolation [3P] and are refused, like every non-Cartesian geometry
static int diff_check(const castro_amd_diffusion* diff, const castro_amd_geom* geom)
{
    if (!diff || !geom) return CASTRO_AMD_ERR_ARG;
    if (geom->coord != 0) return CASTRO_AMD_ERR_UNSUPPORTED;
    for (int d = 0; d < 3; ++d)
        if (geom->lo_bc[d] == 1 || geom->hi_bc[d] == 3) return CASTRO_AMD_ERR_UNSUPPORTED;
    return CASTRO_AMD_OK;
}

static DiffDev to_diffdev(const castro_amd_diffusion* diff, const castro_amd_geom* g)
{
    DiffDev D;
    D.cond = diff->const_conductivity; D.cutoff = diff->diffuse_cutoff_density; D.cutoff_hi = diff->diffuse_cutoff_density_hi;
    D.scale = diff->diffuse_cond_scale_fac;
    for (int d = 0; d < 3; ++d) {
        D.dh[d] = 1.0 / (g->dx[d] * g->dx[d]);
        D.domlo[d] = g->domlo[d]; D.domhi[d] = g->domhi[d];
        D.phys_lo[d] = g->lo_bc[d] != 0 ? 1 : 0;
        D.phys_hi[d] = g->hi_bc[d] != 0 ? 1 : 0;
    }
    return D;
}

// [lo, hi] grown by one inside the FAB: the stencil reads one ghost zone in every direction
static bool fab_contains_grown1(const castro_amd_fab* f, const int lo[3], const int hi[3])
{
    for (int d = 0; d < 3; ++d) if (f->lo[d] > lo[d] - 1 || f->hi[d] < hi[d] + 1) return false;
    return true;
}

static int diff_box(DiffBoxDev& T, const castro_amd_fab* state, const castro_amd_fab* state2, const castro_amd_fab* source,
                    const castro_amd_fab* out, const int lo[3], const int hi[3])
{
    if (!state || !state->p || state->ncomp != NUM_STATE || !fab_contains_grown1(state, lo, hi)) return CASTRO_AMD_ERR_ARG;
    if (state2 && (!state2->p || state2->ncomp != NUM_STATE || !fab_contains_grown1(state2, lo, hi))) return CASTRO_AMD_ERR_ARG;
    if (source && source->p && (source->ncomp <= UEINT || !fab_contains(source, lo, hi))) return CASTRO_AMD_ERR_ARG;
    if (out && out->p && (out->ncomp != 1 || !fab_contains(out, lo, hi))) return CASTRO_AMD_ERR_ARG;
    T.U = to_dfab(state); T.U2 = to_dfab(state2); T.Src = to_dfab(source); T.Out = to_dfab(out);
    for (int d = 0; d < 3; ++d) { T.lo[d] = lo[d]; T.hi[d] = hi[d]; T.nt[d] = 0; }
    return CASTRO_AMD_OK;
}

int castro_amd_temp_diffusion_fab(castro_amd_ctx* c, const castro_amd_fab* state, const castro_amd_fab* source,
                                  const castro_amd_fab* diff_term, const int lo[3], const int hi[3],
                                  const castro_amd_diffusion* diff, const castro_amd_geom* geom, double mult, void* stream)
{
    if (!c || !lo || !hi || ((!source || !source->p) && (!diff_term || !diff_term->p))) return CASTRO_AMD_ERR_ARG;
    int rc = diff_check(diff, geom);
    if (rc != CASTRO_AMD_OK) return rc;
    DiffBoxDev T;
    rc = diff_box(T, state, nullptr, source, diff_term, lo, hi);
    if (rc != CASTRO_AMD_OK) return rc;
    hipSetDevice(c->device);
    return launch_temp_diffusion(1, &T, false, to_diffdev(diff, geom), mult, 0.0, 0, &c->diff_arena, (hipStream_t)stream, &c->prof);
}

int castro_amd_temp_diffusion_mf(castro_amd_ctx* c, int nboxes, const castro_amd_diffusion_box* boxes,
                                 const castro_amd_diffusion* diff, const castro_amd_geom* geom, double mult, void* stream)
{
    if (!c || nboxes < 0 || (nboxes > 0 && !boxes)) return CASTRO_AMD_ERR_ARG;
    int rc = diff_check(diff, geom);
    if (rc != CASTRO_AMD_OK) return rc;
    if (nboxes == 0) return CASTRO_AMD_OK;
    std::vector<DiffBoxDev> tab((size_t)nboxes);
    for (int i = 0; i < nboxes; ++i) {
        if (!boxes[i].source.p) return CASTRO_AMD_ERR_ARG;
        rc = diff_box(tab[(size_t)i], &boxes[i].state, nullptr, &boxes[i].source, nullptr, boxes[i].lo, boxes[i].hi);
        if (rc != CASTRO_AMD_OK) return rc;
    }
    hipSetDevice(c->device);
    return launch_temp_diffusion(nboxes, tab.data(), false, to_diffdev(diff, geom), mult, 0.0, 0, &c->diff_arena, (hipStream_t)stream, &c->prof);
}

int castro_amd_estdt_temp_diffusion_fab(castro_amd_ctx* c, const castro_amd_fab* state, const int lo[3], const int hi[3],
                                        const castro_amd_geom* geom, const castro_amd_params* params,
                                        const castro_amd_diffusion* diff, double max_dt, double* d_out, void* stream)
{
    if (!c || !state || !state->p || !lo || !hi || !geom || !params || !diff || !d_out || state->ncomp != NUM_STATE) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_estdt_temp_diffusion(to_dfab(state), lo, hi, geom->dx, to_devparams(params), diff->const_conductivity,
                                       diff->diffuse_cutoff_density, max_dt / params->cfl, d_out, (hipStream_t)stream, &c->prof);
}

int castro_amd_estdt_temp_diffusion_mf(castro_amd_ctx* c, int nboxes, const castro_amd_state_box* boxes, const castro_amd_geom* geom,
                                       const castro_amd_params* params, const castro_amd_diffusion* diff, double max_dt,
                                       double* d_out, void* stream)
{
    if (!c || nboxes < 0 || (nboxes > 0 && !boxes)) return CASTRO_AMD_ERR_ARG;
    for (int i = 0; i < nboxes; ++i) {
        const int rc = castro_amd_estdt_temp_diffusion_fab(c, &boxes[i].state, boxes[i].lo, boxes[i].hi, geom, params, diff, max_dt, d_out, stream);
        if (rc != CASTRO_AMD_OK) return rc;
    }
    return CASTRO_AMD_OK;
}

// the checks of castro_amd_new_sponge_source_fab; stage 0 takes a sponge and adds nothing
static bool sponge_ok(const castro_amd_sponge* sponge, const castro_amd_geom* geom, double dt)
{
    return !sponge || (geom->coord == 0 && dt > 0.0 && sponge->timescale > 0.0);
}

static bool grav_fab_ok(const castro_amd_fab* g, const int lo[3], const int hi[3], int grav_source_type);

// the checks of one box of the one-pass sources, and the box as the kernel reads it
static int src_box(SrcBoxDev& T, const castro_amd_source_box& b, bool mass_fluxes)
{
    if (!b.S_old.p || !b.S_new.p || !b.source.p || b.S_old.ncomp != NUM_STATE || b.S_new.ncomp != NUM_STATE || b.source.ncomp < 7)
        return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(&b.S_old, b.lo, b.hi) || !fab_contains(&b.S_new, b.lo, b.hi) || !fab_contains(&b.source, b.lo, b.hi)) return CASTRO_AMD_ERR_ARG;
    T.So = to_dfab(&b.S_old); T.Sn = to_dfab(&b.S_new); T.Src = to_dfab(&b.source);
    T.M0 = T.M1 = T.M2 = to_dfab(nullptr);
    if (mass_fluxes) {
        DFab M[3];
        if (!mass_flux_dfabs(b.mass_flux, b.lo, b.hi, M)) return CASTRO_AMD_ERR_ARG;
        T.M0 = M[0]; T.M1 = M[1]; T.M2 = M[2];
    }
    for (int d = 0; d < 3; ++d) {
        if (b.source.hi[d] < b.source.lo[d]) return CASTRO_AMD_ERR_ARG;
        T.lo[d] = b.source.lo[d]; T.n[d] = b.source.hi[d] - b.source.lo[d] + 1;
        T.vlo[d] = b.lo[d]; T.vhi[d] = b.hi[d];
    }
    T.nsc = b.source.ncomp;
    return CASTRO_AMD_OK;
}

// The one-pass sources behind their four entry points.  Gravity is a vector for the level (o.grav) or one FAB per box
// (o.grav_old / o.grav_new), not both; the FABs do not go together with diffusion.
static int sources_mf_impl(castro_amd_ctx* c, int stage_arg, int nboxes, const castro_amd_source_box* boxes, const castro_amd_source_opts& o,
                           const castro_amd_geom* geom, const castro_amd_params* params, double dt, int clean_ntimes, void* stream)
{
    // the kernel's stage: 0, 1, or 2 for stage 1 with CASTRO_AMD_SOURCES_AFTER_REFLUX; any other value of the argument
    // (the bare 2 included) is refused below
    const int stage = stage_arg == (1 | CASTRO_AMD_SOURCES_AFTER_REFLUX) ? 2 : (stage_arg == 0 || stage_arg == 1) ? stage_arg : -1;
    const bool gfab = o.grav_old || o.grav_new, grav_on = gfab || o.grav;
    if (gfab && o.grav) return CASTRO_AMD_ERR_ARG;
    if (gfab && o.diff) return CASTRO_AMD_ERR_UNSUPPORTED;
    if (!c || stage < 0 || nboxes < 0 || (nboxes > 0 && !boxes) || !geom || !params || clean_ntimes < 0) return CASTRO_AMD_ERR_ARG;
    // after a reflux: stage 1 behind the removal of the stored source; the stencil of the diffusion term would read neighbours that
    // other threads of the one pass are rewriting
    if (stage == 2 && o.diff) return CASTRO_AMD_ERR_UNSUPPORTED;
    const bool newt = stage >= 1;          // the new-time source functions
    if (!sponge_ok(o.sponge, geom, dt)) return CASTRO_AMD_ERR_ARG;
    if (gfab && nboxes > 0 && (!o.grav_old || (newt && !o.grav_new))) return CASTRO_AMD_ERR_ARG;
    // the checks of the single-box entry points (castro_amd_old/new_gravity_source_fab, _rotation_source_fab, _apply_source_fab)
    if (grav_on && (o.grav_source_type < 1 || o.grav_source_type > 4)) return CASTRO_AMD_ERR_ARG;
    if (o.rot && (o.rot->rot_source_type < 1 || o.rot->rot_source_type > 4)) return CASTRO_AMD_ERR_ARG;
    if ((o.rot || (grav_on && newt)) && geom->coord != 0) return CASTRO_AMD_ERR_ARG;
    if (o.rot && newt && !(dt > 0.0)) return CASTRO_AMD_ERR_ARG;
    if (o.diff) {
        const int rc = diff_check(o.diff, geom);
        if (rc != CASTRO_AMD_OK) return rc;
    }
    if (nboxes == 0) return CASTRO_AMD_OK;
    std::vector<SrcBoxDev> tab(gfab ? 0 : (size_t)nboxes);
    std::vector<SrcBoxGDev> gtab(gfab ? (size_t)nboxes : 0);
    std::vector<DiffBoxDev> dtab(o.diff ? (size_t)nboxes : 0);
    for (int i = 0; i < nboxes; ++i) {
        const castro_amd_source_box& b = boxes[i];
        const int rb = src_box(gfab ? gtab[(size_t)i].box : tab[(size_t)i], b, newt && (grav_on || o.rot));
        if (rb != CASTRO_AMD_OK) return rb;
        if (gfab) {
            // stage 0 reads the zone itself, stage 1 with grav_source_type 4 its six neighbours as well
            if (!grav_fab_ok(&o.grav_old[i], b.lo, b.hi, newt ? o.grav_source_type : 1)) return CASTRO_AMD_ERR_ARG;
            if (newt && !grav_fab_ok(&o.grav_new[i], b.lo, b.hi, o.grav_source_type)) return CASTRO_AMD_ERR_ARG;
            gtab[(size_t)i].GO = to_dfab(&o.grav_old[i]);
            gtab[(size_t)i].GN = to_dfab(newt ? &o.grav_new[i] : &o.grav_old[i]);
        }
        // diff_src: stage 0 the term of S_old, stage 1 the corrector 0.5 DiffTerm(S_new) - 0.5 DiffTerm(S_old)
        if (o.diff) {
            const int rd = stage == 0 ? diff_box(dtab[(size_t)i], &b.S_old, nullptr, &b.source, nullptr, b.lo, b.hi)
                                      : diff_box(dtab[(size_t)i], &b.S_new, &b.S_old, &b.source, nullptr, b.lo, b.hi);
            if (rd != CASTRO_AMD_OK) return rd;
        }
    }
    hipSetDevice(c->device);
    if (o.diff) {
        // a launch of its own in front of the one-pass kernel: that kernel writes S_new in place, and the stencil of the
        // new-time term reads the neighbours' S_new.  It leaves 0 + term in UEDEN / UEINT of the valid zones; the one-pass
        // kernel starts its sums of those two components from there instead of from zero.
        const int rd = launch_temp_diffusion(nboxes, dtab.data(), stage == 1, to_diffdev(o.diff, geom), stage == 0 ? 1.0 : 0.5, -0.5, 1,
                                             &c->diff_arena, (hipStream_t)stream, &c->prof);
        if (rd != 0) return rd;
    }
    const DevParams P = to_devparams(params);
    return gfab ? launch_sources_apply_gfab(stage, nboxes, gtab.data(), o.grav_source_type, o.rot, geom, P, dt, clean_ntimes, &c->ops_arena,
                                            (hipStream_t)stream, &c->prof, 0, o.sponge)
                : launch_sources_apply(stage, nboxes, tab.data(), o.grav, o.grav_source_type, o.rot, geom, P, dt, clean_ntimes, &c->ops_arena,
                                       (hipStream_t)stream, &c->prof, o.diff ? 1 : 0, o.sponge);
}

int castro_amd_sources_mf(castro_amd_ctx* c, int stage, int nboxes, const castro_amd_source_box* boxes,
                          const double* grav, int grav_source_type, const castro_amd_rotation* rot,
                          const castro_amd_geom* geom, const castro_amd_params* params, double dt, int clean_ntimes, void* stream)
{
    return castro_amd_sources_mf_ex(c, stage, nboxes, boxes, grav, grav_source_type, rot, nullptr, geom, params, dt, clean_ntimes, stream);
}

int castro_amd_sources_mf_ex(castro_amd_ctx* c, int stage, int nboxes, const castro_amd_source_box* boxes,
                             const double* grav, int grav_source_type, const castro_amd_rotation* rot,
                             const castro_amd_diffusion* diff, const castro_amd_geom* geom, const castro_amd_params* params,
                             double dt, int clean_ntimes, void* stream)
{
    const castro_amd_source_opts o = { grav, nullptr, nullptr, grav_source_type, rot, diff, nullptr };
    return sources_mf_impl(c, stage, nboxes, boxes, o, geom, params, dt, clean_ntimes, stream);
}

int castro_amd_sources_mf_g(castro_amd_ctx* c, int stage, int nboxes, const castro_amd_source_box* boxes,
                            const castro_amd_fab* grav_old, const castro_amd_fab* grav_new, int grav_source_type,
                            const castro_amd_rotation* rot, const castro_amd_geom* geom, const castro_amd_params* params,
                            double dt, int clean_ntimes, void* stream)
{
    castro_amd_source_opts o = { nullptr, grav_old, grav_new, grav_source_type, rot, nullptr, nullptr };
    // without either array the call is still the FAB form, with that form's checks: refused unless the level is empty
    static const castro_amd_fab none = { nullptr, { 0, 0, 0 }, { 0, 0, 0 }, 0 };
    if (!grav_old && !grav_new) {
        if (nboxes > 0) return CASTRO_AMD_ERR_ARG;
        o.grav_old = &none;
    }
    return sources_mf_impl(c, stage, nboxes, boxes, o, geom, params, dt, clean_ntimes, stream);
}

int castro_amd_sources_mf_opts(castro_amd_ctx* c, int stage, int nboxes, const castro_amd_source_box* boxes,
                               const castro_amd_source_opts* o, const castro_amd_geom* geom, const castro_amd_params* params,
                               double dt, int clean_ntimes, void* stream)
{
    if (!o) return CASTRO_AMD_ERR_ARG;
    return sources_mf_impl(c, stage, nboxes, boxes, *o, geom, params, dt, clean_ntimes, stream);
}

int castro_amd_clean_state_reduce_mf(castro_amd_ctx* c, int nboxes, const castro_amd_state_box* boxes, const castro_amd_geom* geom,
                                     const castro_amd_params* params, int ntimes, double* d_out, void* stream)
{
    if (!c || nboxes < 0 || (nboxes > 0 && !boxes)) return CASTRO_AMD_ERR_ARG;
    for (int i = 0; i < nboxes; ++i) {
        const int rc = castro_amd_clean_state_reduce_fab(c, &boxes[i].state, boxes[i].lo, boxes[i].hi, geom, params, ntimes, d_out, stream);
        if (rc != CASTRO_AMD_OK) return rc;
    }
    return CASTRO_AMD_OK;
}

int castro_amd_estdt_mf(castro_amd_ctx* c, int nboxes, const castro_amd_state_box* boxes, const castro_amd_geom* geom,
                        const castro_amd_params* params, double* d_out, void* stream)
{
    if (!c || nboxes < 0 || (nboxes > 0 && !boxes)) return CASTRO_AMD_ERR_ARG;
    for (int i = 0; i < nboxes; ++i) {
        const int rc = castro_amd_estdt_fab(c, &boxes[i].state, boxes[i].lo, boxes[i].hi, geom, params, d_out, stream);
        if (rc != CASTRO_AMD_OK) return rc;
    }
    return CASTRO_AMD_OK;
}

// the checks of castro_amd_integrated_quantities_mf on its box table, and the table the kernels read
static int diag_table(int nboxes, const castro_amd_diag_box* boxes, std::vector<DiagBoxDev>& tab)
{
    if (nboxes < 0 || (nboxes > 0 && !boxes)) return CASTRO_AMD_ERR_ARG;
    tab.resize((size_t)nboxes);
    for (int i = 0; i < nboxes; ++i) {
        const castro_amd_diag_box& b = boxes[i];
        if (!b.state.p || b.state.ncomp != NUM_STATE || !fab_contains(&b.state, b.lo, b.hi)) return CASTRO_AMD_ERR_ARG;
        DiagBoxDev& T = tab[(size_t)i];
        T.U = to_dfab(&b.state);
        T.mask = b.mask;
        for (int d = 0; d < 3; ++d) { T.lo[d] = b.lo[d]; T.n[d] = b.hi[d] - b.lo[d] + 1; }
        T.npr = 0;
    }
    return CASTRO_AMD_OK;
}

int castro_amd_integrated_quantities_mf(castro_amd_ctx* c, int nboxes, const castro_amd_diag_box* boxes, const castro_amd_geom* geom,
                                        const double center[3], double* d_out, void* stream)
{
    if (!c || !geom || !center || !d_out) return CASTRO_AMD_ERR_ARG;
    if (geom->coord != 0) return CASTRO_AMD_ERR_UNSUPPORTED;
    std::vector<DiagBoxDev> tab;
    const int rt = diag_table(nboxes, boxes, tab);
    if (rt != CASTRO_AMD_OK) return rt;
    DiagGeom G;
    for (int d = 0; d < 3; ++d) { G.dx[d] = geom->dx[d]; G.problo[d] = geom->problo[d]; G.center[d] = center[d]; }
    G.vol = geom->dx[0] * geom->dx[1] * geom->dx[2];
    hipSetDevice(c->device);
    return launch_integrated_quantities(nboxes, tab.data(), G, &c->diag_arena, &c->diag_ws, d_out, (hipStream_t)stream, &c->prof);
}

// the checks of castro_amd_fab_pack / castro_amd_fab_unpack on their table, and the table the kernels read
static int pack_table(int n, const castro_amd_pack_entry* entries, const double* buf, std::vector<PackEntryDev>& tab)
{
    tab.resize((size_t)n);
    const bool buf16 = (reinterpret_cast<uintptr_t>(buf) & 15u) == 0;
    for (int i = 0; i < n; ++i) {
        const castro_amd_pack_entry& e = entries[i];
        if (!e.fab.p || e.fab.ncomp < 1 || e.offset < 0) return CASTRO_AMD_ERR_ARG;
        for (int d = 0; d < 3; ++d) if (e.vhi[d] < e.vlo[d]) return CASTRO_AMD_ERR_ARG;
        if (!fab_contains(&e.fab, e.vlo, e.vhi)) return CASTRO_AMD_ERR_ARG;
        const DFab F = to_dfab(&e.fab);
        PackEntryDev& T = tab[(size_t)i];
        long zones = 1;
        for (int d = 0; d < 3; ++d) { T.n[d] = e.vhi[d] - e.vlo[d] + 1; zones *= T.n[d]; }
        if (zones > 0x7fffffffL) return CASTRO_AMD_ERR_ARG;      // the kernels divide 32-bit zone numbers
        T.p = F.p + (long)(e.vlo[0] - F.lo[0]) + F.sy * (long)(e.vlo[1] - F.lo[1]) + F.sz * (long)(e.vlo[2] - F.lo[2]);
        T.sy = F.sy; T.sz = F.sz; T.sn = F.sn;
        T.offset = (long)e.offset;
        T.zones = zones;
        T.ncomp = e.fab.ncomp;
        T.bpc = 0;
        T.vec2 = (buf16 && (reinterpret_cast<uintptr_t>(T.p) & 15u) == 0 && T.n[0] % 2 == 0 && F.sy % 2 == 0 && F.sz % 2 == 0 &&
                  F.sn % 2 == 0 && e.offset % 2 == 0) ? 1 : 0;
        T.items = T.vec2 ? zones / 2 : zones;
    }
    return CASTRO_AMD_OK;
}

int castro_amd_fab_pack(castro_amd_ctx* c, int n, const castro_amd_pack_entry* entries, double* d_dst, double* d_minmax, void* stream)
{
    if (!c || n < 0) return CASTRO_AMD_ERR_ARG;
    if (n == 0) return CASTRO_AMD_OK;
    if (!entries || !d_dst) return CASTRO_AMD_ERR_ARG;
    std::vector<PackEntryDev> tab;
    const int rt = pack_table(n, entries, d_dst, tab);
    if (rt != CASTRO_AMD_OK) return rt;
    hipSetDevice(c->device);
    return launch_fab_pack(0, n, tab.data(), &c->pack_arena, &c->pack_ws, d_dst, d_minmax, (hipStream_t)stream, &c->prof);
}

int castro_amd_fab_unpack(castro_amd_ctx* c, int n, const castro_amd_pack_entry* entries, const double* d_src, void* stream)
{
    if (!c || n < 0) return CASTRO_AMD_ERR_ARG;
    if (n == 0) return CASTRO_AMD_OK;
    if (!entries || !d_src) return CASTRO_AMD_ERR_ARG;
    std::vector<PackEntryDev> tab;
    const int rt = pack_table(n, entries, d_src, tab);
    if (rt != CASTRO_AMD_OK) return rt;
    hipSetDevice(c->device);
    return launch_fab_pack(1, n, tab.data(), &c->pack_arena, &c->pack_ws, const_cast<double*>(d_src), nullptr, (hipStream_t)stream,
                           &c->prof);
}

int castro_amd_diag_workgroups(int nboxes, const castro_amd_diag_box* boxes)
{
    std::vector<DiagBoxDev> tab;
    const int rt = diag_table(nboxes, boxes, tab);
    if (rt != CASTRO_AMD_OK) return rt;
    if (nboxes == 0) return 0;
    std::vector<int> start;
    int iters = 0;
    const int rc = diag_layout(nboxes, tab.data(), start, iters);
    return rc != 0 ? rc : start.back();
}

// castro_amd_monopole_params + castro_amd_geom as the kernels read them
static int mono_geom(const castro_amd_geom* geom, const castro_amd_monopole_params* mp, MonoGeom& G)
{
    if (!geom || !mp || mp->n1d < 2 || mp->drdxfac < 1) return CASTRO_AMD_ERR_ARG;
    if (geom->coord != 0) return CASTRO_AMD_ERR_UNSUPPORTED;
    bool octant = true;
    for (int d = 0; d < 3; ++d) {
        if (!(geom->dx[d] > 0.0)) return CASTRO_AMD_ERR_ARG;
        G.dx[d] = geom->dx[d]; G.problo[d] = geom->problo[d]; G.center[d] = mp->center[d];
        octant = octant && std::fabs(mp->center[d] - geom->problo[d]) < 1.e-2 * geom->dx[d];        // Gravity.cpp:1439-1447
    }
    G.octant_factor = octant ? 8.0 : 1.0;
    G.max_radius = mp->max_radius_all_in_domain;
    G.Gconst = mp->Gconst;
    G.n1d = mp->n1d; G.drdxfac = mp->drdxfac;
    return CASTRO_AMD_OK;
}

int castro_amd_radial_mass_mf(castro_amd_ctx* c, int nboxes, const castro_amd_diag_box* boxes, const castro_amd_geom* geom,
                              const castro_amd_monopole_params* params, double* d_mass_vol, void* stream)
{
    if (!c || !d_mass_vol || nboxes < 0 || (nboxes > 0 && !boxes)) return CASTRO_AMD_ERR_ARG;
    MonoGeom G;
    const int rg = mono_geom(geom, params, G);
    if (rg != CASTRO_AMD_OK) return rg;
    // the table is compared byte by byte with the ones already on the device: every byte of it is set here
    std::vector<MonoBoxDev> tab((size_t)nboxes);
    if (nboxes > 0) std::memset((void*)tab.data(), 0, (size_t)nboxes * sizeof(MonoBoxDev));
    for (int i = 0; i < nboxes; ++i) {
        const castro_amd_diag_box& b = boxes[i];
        if (!b.state.p || b.state.ncomp != NUM_STATE || !fab_contains(&b.state, b.lo, b.hi)) return CASTRO_AMD_ERR_ARG;
        MonoBoxDev& T = tab[(size_t)i];
        const DFab U = to_dfab(&b.state);
        T.U.p = U.p; T.U.sy = U.sy; T.U.sz = U.sz; T.U.sn = U.sn;
        T.mask = b.mask;
        for (int d = 0; d < 3; ++d) { T.U.lo[d] = U.lo[d]; T.lo[d] = b.lo[d]; T.n[d] = b.hi[d] - b.lo[d] + 1; }
    }
    hipSetDevice(c->device);
    return launch_radial_mass(nboxes, tab.data(), G, &c->mono_ws, d_mass_vol, (hipStream_t)stream, &c->prof);
}

int castro_amd_radial_mass_mf_ex(castro_amd_ctx* c, int nboxes, const castro_amd_radial_box* boxes, const castro_amd_geom* geom,
                                 const castro_amd_monopole_params* params, double* d_mass_vol, void* stream)
{
    if (!c || !d_mass_vol || nboxes < 0 || (nboxes > 0 && !boxes)) return CASTRO_AMD_ERR_ARG;
    MonoGeom G;
    const int rg = mono_geom(geom, params, G);
    if (rg != CASTRO_AMD_OK) return rg;
    // compared byte by byte with the tables already on the device: every byte is set here
    std::vector<MonoBoxDevEx> tab((size_t)nboxes);
    if (nboxes > 0) std::memset((void*)tab.data(), 0, (size_t)nboxes * sizeof(MonoBoxDevEx));
    for (int i = 0; i < nboxes; ++i) {
        const castro_amd_radial_box& b = boxes[i];
        if (!b.state_old.p || b.state_old.ncomp != NUM_STATE || !fab_contains(&b.state_old, b.lo, b.hi)) return CASTRO_AMD_ERR_ARG;
        if (!b.state_new.p || b.state_new.ncomp != NUM_STATE || !fab_contains(&b.state_new, b.lo, b.hi)) return CASTRO_AMD_ERR_ARG;
        MonoBoxDevEx& T = tab[(size_t)i];
        const DFab U = to_dfab(&b.state_old), U2 = to_dfab(&b.state_new);
        T.U.p = U.p; T.U.sy = U.sy; T.U.sz = U.sz; T.U.sn = U.sn;
        T.U2.p = U2.p; T.U2.sy = U2.sy; T.U2.sz = U2.sz; T.U2.sn = U2.sn;
        T.mask = b.mask;
        T.omalpha = b.omalpha; T.alpha = b.alpha;
        for (int d = 0; d < 3; ++d) { T.U.lo[d] = U.lo[d]; T.U2.lo[d] = U2.lo[d]; T.lo[d] = b.lo[d]; T.n[d] = b.hi[d] - b.lo[d] + 1; }
    }
    hipSetDevice(c->device);
    return launch_radial_mass_ex(nboxes, tab.data(), G, &c->mono_ws, d_mass_vol, (hipStream_t)stream, &c->prof);
}

int castro_amd_radial_combine(castro_amd_ctx* c, int level, const double* const* d_mass_vol, const int* n1d, double* d_out, void* stream)
{
    if (!c || level < 0 || level >= MONO_MAX_LEVELS || !d_mass_vol || !n1d || !d_out) return CASTRO_AMD_ERR_ARG;
    MonoCombine A;
    std::memset(&A, 0, sizeof(A));
    A.level = level;
    for (int l = 0; l <= level; ++l) { A.mv[l] = d_mass_vol[l]; A.n1d[l] = n1d[l]; }
    hipSetDevice(c->device);
    return launch_radial_combine(A, d_out, (hipStream_t)stream, &c->prof);
}

int castro_amd_grav_bc_fill_fab(castro_amd_ctx* c, const castro_amd_fab* grav_fab, const castro_amd_geom* geom, void* stream)
{
    if (!c || !grav_fab || !grav_fab->p || grav_fab->ncomp != 3 || !geom) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_grav_bc_fill(to_dfab(grav_fab), grav_fab->lo, grav_fab->hi, geom->domlo, geom->domhi, geom->lo_bc, geom->hi_bc,
                               (hipStream_t)stream, &c->prof);
}

int castro_amd_radial_gravity(castro_amd_ctx* c, const castro_amd_monopole_params* params, const castro_amd_geom* geom,
                              const double* d_mass_vol, double* d_radial_grav, void* stream)
{
    if (!c || !d_mass_vol || !d_radial_grav) return CASTRO_AMD_ERR_ARG;
    MonoGeom G;
    const int rg = mono_geom(geom, params, G);
    if (rg != CASTRO_AMD_OK) return rg;
    hipSetDevice(c->device);
    return launch_radial_gravity(G, d_mass_vol, d_radial_grav, (hipStream_t)stream, &c->prof);
}

int castro_amd_monopole_grav_fab(castro_amd_ctx* c, const double* d_radial_grav, const castro_amd_monopole_params* params,
                                 const castro_amd_geom* geom, const castro_amd_fab* grav_fab, void* stream)
{
    if (!c || !d_radial_grav || !grav_fab || !grav_fab->p || grav_fab->ncomp != 3) return CASTRO_AMD_ERR_ARG;
    MonoGeom G;
    const int rg = mono_geom(geom, params, G);
    if (rg != CASTRO_AMD_OK) return rg;
    hipSetDevice(c->device);
    return launch_monopole_grav(d_radial_grav, G, to_dfab(grav_fab), grav_fab->lo, grav_fab->hi, (hipStream_t)stream, &c->prof);
}

// ---- Poisson gravity on a single level (poisson_kernels.hip) -------------------------------------------------------------------
// Cartesian, and every face a Dirichlet face of the potential: not periodic / interior (0), not Symmetry (3)
static int poisson_geom_ok(const castro_amd_geom* geom)
{
    if (!geom) return CASTRO_AMD_ERR_ARG;
    if (geom->coord != 0) return CASTRO_AMD_ERR_UNSUPPORTED;
    for (int d = 0; d < 3; ++d) {
        if (!(geom->dx[d] > 0.0) || geom->domhi[d] < geom->domlo[d]) return CASTRO_AMD_ERR_ARG;
        if (geom->lo_bc[d] == 0 || geom->hi_bc[d] == 0 || geom->lo_bc[d] == 3 || geom->hi_bc[d] == 3) return CASTRO_AMD_ERR_UNSUPPORTED;
    }
    return CASTRO_AMD_OK;
}

static int mp_geom(const castro_amd_geom* geom, const castro_amd_multipole* mp, MpGeom& G)
{
    if (!mp) return CASTRO_AMD_ERR_ARG;
    const int rg = poisson_geom_ok(geom);
    if (rg != CASTRO_AMD_OK) return rg;
    if (mp->lnum < 0 || !(mp->rmax > 0.0)) return CASTRO_AMD_ERR_ARG;
    if (mp->lnum > CASTRO_AMD_MAX_MULTIPOLE) return CASTRO_AMD_ERR_UNSUPPORTED;
    for (int d = 0; d < 3; ++d) {
        G.dx[d] = geom->dx[d]; G.problo[d] = geom->problo[d]; G.center[d] = mp->center[d];
        G.domlo[d] = geom->domlo[d]; G.domhi[d] = geom->domhi[d];
    }
    G.rmax = mp->rmax; G.Gconst = mp->Gconst; G.lnum = mp->lnum;
    return CASTRO_AMD_OK;
}

int castro_amd_multipole_moments_mf(castro_amd_ctx* c, int nboxes, const castro_amd_diag_box* boxes, const castro_amd_geom* geom,
                                    const castro_amd_multipole* mp, double* d_moments, void* stream)
{
    if (!c || !d_moments) return CASTRO_AMD_ERR_ARG;
    MpGeom G;
    const int rg = mp_geom(geom, mp, G);
    if (rg != CASTRO_AMD_OK) return rg;
    std::vector<DiagBoxDev> tab;
    const int rt = diag_table(nboxes, boxes, tab);
    if (rt != CASTRO_AMD_OK) return rt;
    hipSetDevice(c->device);
    return launch_multipole_moments(nboxes, tab.data(), G, &c->mp_arena, &c->mp_ws, d_moments, (hipStream_t)stream, &c->prof);
}

int castro_amd_multipole_phi_bc_fab(castro_amd_ctx* c, const castro_amd_fab* phi_fab, const castro_amd_geom* geom,
                                    const castro_amd_multipole* mp, const double* d_moments, void* stream)
{
    if (!c || !phi_fab || !phi_fab->p || phi_fab->ncomp != 1 || !d_moments) return CASTRO_AMD_ERR_ARG;
    MpGeom G;
    const int rg = mp_geom(geom, mp, G);
    if (rg != CASTRO_AMD_OK) return rg;
    for (int d = 0; d < 3; ++d) if (phi_fab->hi[d] < phi_fab->lo[d]) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_multipole_phi_bc(to_dfab(phi_fab), phi_fab->lo, phi_fab->hi, G, d_moments, (hipStream_t)stream, &c->prof);
}

int castro_amd_poisson_plan_create(castro_amd_ctx* c, const castro_amd_geom* geom, castro_amd_poisson_plan** plan)
{
    if (!c || !plan) return CASTRO_AMD_ERR_ARG;
    const int rg = poisson_geom_ok(geom);
    if (rg != CASTRO_AMD_OK) return rg;
    int n[3];
    for (int d = 0; d < 3; ++d) n[d] = geom->domhi[d] - geom->domlo[d] + 1;
    // the level table first: a refusal costs no device memory (and needs no device)
    std::vector<MgLevel> lev;
    const int rl = poisson_levels(n, geom->domlo, geom->dx, lev);
    if (rl != 0) return rl;
    hipSetDevice(c->device);
    PoissonPlan* P = nullptr;
    const int rc = poisson_plan_make(n, geom->domlo, geom->dx, &P);
    if (rc != 0) return rc;
    *plan = reinterpret_cast<castro_amd_poisson_plan*>(P);
    return CASTRO_AMD_OK;
}

void castro_amd_poisson_plan_destroy(castro_amd_ctx* c, castro_amd_poisson_plan* plan)
{
    if (!c || !plan) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    poisson_plan_free(reinterpret_cast<PoissonPlan*>(plan));
}

// does `f` hold the box of level L grown by ng zones?
static bool mg_fab_ok(const castro_amd_fab* f, const MgLevel& L, int ng)
{
    if (!f || !f->p || f->ncomp < 1) return false;
    int lo[3], hi[3];
    for (int d = 0; d < 3; ++d) { lo[d] = L.lo[d] - ng; hi[d] = L.lo[d] + L.n[d] - 1 + ng; }
    return fab_contains(f, lo, hi);
}

int castro_amd_poisson_solve(castro_amd_ctx* c, castro_amd_poisson_plan* plan, const castro_amd_fab* phi_fab,
                             const castro_amd_fab* rho_fab, int rho_comp, double fourpiG, double reltol, double abstol, int maxiter,
                             int* cycles, int* converged, double* final_norm, double* h_history, void* stream)
{
    if (!c || !plan || !cycles || !converged || !final_norm || maxiter < 0) return CASTRO_AMD_ERR_ARG;
    PoissonPlan* P = reinterpret_cast<PoissonPlan*>(plan);
    if (!P->flags.empty()) return CASTRO_AMD_ERR_ARG;      // the plan of a union of boxes: castro_amd_poisson_boxes_solve
    const MgLevel& L0 = P->lev[0];
    if (!mg_fab_ok(phi_fab, L0, 1) || phi_fab->ncomp != 1 || !mg_fab_ok(rho_fab, L0, 0)) return CASTRO_AMD_ERR_ARG;
    if (rho_comp < 0 || rho_comp >= rho_fab->ncomp) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_poisson_solve(P, to_dfab(phi_fab), to_dfab(rho_fab), rho_comp, fourpiG, reltol, abstol, maxiter, cycles, converged,
                                final_norm, h_history, (hipStream_t)stream, &c->prof);
}

// one pass on the level `level` (inside the plan) of a plan of either kind; e: the edge of that level, cflags: the coverage of the
// next coarser level of a union, or nullptr
static int mg_level_op(castro_amd_ctx* c, PoissonPlan* P, int op, int level, int colour, const castro_amd_fab* a, const castro_amd_fab* b,
                       const castro_amd_fab* f3, const MgEdge& e, const unsigned char* cflags, double* d_out, void* stream)
{
    const int nl = (int)P->lev.size();
    const MgLevel& L = P->lev[(size_t)level];
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(c->device);
    switch (op) {
    case CASTRO_AMD_MG_SMOOTH:
        if ((colour != 0 && colour != 1) || !mg_fab_ok(a, L, 1) || !mg_fab_ok(b, L, 0)) return CASTRO_AMD_ERR_ARG;
        return launch_mg_smooth(to_dfab(a), to_dfab(b), L, e, colour, s, &c->prof);
    case CASTRO_AMD_MG_RESIDUAL:
        if (!mg_fab_ok(a, L, 1) || !mg_fab_ok(b, L, 0) || !mg_fab_ok(f3, L, 0)) return CASTRO_AMD_ERR_ARG;
        return launch_mg_residual(to_dfab(a), to_dfab(b), to_dfab(f3), L, e, s, &c->prof);
    case CASTRO_AMD_MG_RESTRICT:
        if (level + 1 >= nl) return CASTRO_AMD_ERR_ARG;
        if (!mg_fab_ok(a, L, 0) || !mg_fab_ok(b, P->lev[(size_t)level + 1], 0) || !mg_fab_ok(f3, P->lev[(size_t)level + 1], 0)) return CASTRO_AMD_ERR_ARG;
        return launch_mg_restrict(to_dfab(a), L, to_dfab(b), to_dfab(f3), P->lev[(size_t)level + 1], cflags, s, &c->prof);
    case CASTRO_AMD_MG_PROLONG:
        if (level + 1 >= nl) return CASTRO_AMD_ERR_ARG;
        if (!mg_fab_ok(a, P->lev[(size_t)level + 1], 0) || !mg_fab_ok(b, L, 0)) return CASTRO_AMD_ERR_ARG;
        return launch_mg_prolong(to_dfab(a), P->lev[(size_t)level + 1], to_dfab(b), L, e.flags, s, &c->prof);
    case CASTRO_AMD_MG_NORM:
        if (!mg_fab_ok(a, L, 0) || !d_out) return CASTRO_AMD_ERR_ARG;
        return launch_mg_norm(to_dfab(a), L, e.flags, P->norm_ws, d_out, s, &c->prof);
    default:
        return CASTRO_AMD_ERR_ARG;
    }
}

int castro_amd_poisson_level_op(castro_amd_ctx* c, castro_amd_poisson_plan* plan, int op, int level, int colour,
                                const castro_amd_fab* a, const castro_amd_fab* b, const castro_amd_fab* f3, double* d_out, void* stream)
{
    if (!c || !plan) return CASTRO_AMD_ERR_ARG;
    PoissonPlan* P = reinterpret_cast<PoissonPlan*>(plan);
    if (level < 0 || level >= (int)P->lev.size() || !P->flags.empty()) return CASTRO_AMD_ERR_ARG;
    MgEdge e;
    std::memset(&e, 0, sizeof(e));
    return mg_level_op(c, P, op, level, colour, a, b, f3, e, nullptr, d_out, stream);
}

int castro_amd_grad_phi_to_grav_fab(castro_amd_ctx* c, const castro_amd_fab* phi_fab, const castro_amd_fab* grav_fab,
                                    const castro_amd_geom* geom, void* stream)
{
    if (!c) return CASTRO_AMD_ERR_ARG;
    const int rg = poisson_geom_ok(geom);
    if (rg != CASTRO_AMD_OK) return rg;
    MgLevel L;
    std::memset(&L, 0, sizeof(L));
    for (int d = 0; d < 3; ++d) { L.lo[d] = geom->domlo[d]; L.n[d] = geom->domhi[d] - geom->domlo[d] + 1; }
    if (!mg_fab_ok(phi_fab, L, 1) || phi_fab->ncomp != 1 || !mg_fab_ok(grav_fab, L, 0) || grav_fab->ncomp != 3) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_grad_phi(to_dfab(phi_fab), to_dfab(grav_fab), L, geom->dx, (hipStream_t)stream, &c->prof);
}

// the Dirichlet data of a refined level's own solve: the fine box (ratio 2: even low, odd high corner) grown by one inside
// phi_fine_fab, the coarsened box grown by one inside both coarse FABs
int castro_amd_poisson_cf_bc_fab(castro_amd_ctx* c, const castro_amd_fab* phi_fine_fab, const int fine_lo[3], const int fine_hi[3],
                                 const castro_amd_fab* crse_old_fab, const castro_amd_fab* crse_new_fab, double a, void* stream)
{
    if (!c || !fine_lo || !fine_hi || !(a - a == 0.0)) return CASTRO_AMD_ERR_ARG;
    const castro_amd_fab* fabs[3] = { phi_fine_fab, crse_old_fab, crse_new_fab };
    for (const castro_amd_fab* f : fabs) {
        if (!f || !f->p || f->ncomp != 1) return CASTRO_AMD_ERR_ARG;
        for (int d = 0; d < 3; ++d) if (f->hi[d] < f->lo[d]) return CASTRO_AMD_ERR_ARG;
    }
    int clo[3], chi[3];
    for (int d = 0; d < 3; ++d) {
        if (fine_hi[d] < fine_lo[d] || (fine_lo[d] & 1) != 0 || (fine_hi[d] & 1) != 1) return CASTRO_AMD_ERR_ARG;
        if (fine_lo[d] < -(1 << 30) || fine_hi[d] > (1 << 30)) return CASTRO_AMD_ERR_ARG;
        clo[d] = (fine_lo[d] >> 1) - 1;
        chi[d] = (fine_hi[d] >> 1) + 1;
    }
    if (!fab_contains_grown1(phi_fine_fab, fine_lo, fine_hi) || !fab_contains(crse_old_fab, clo, chi) || !fab_contains(crse_new_fab, clo, chi))
        return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_phi_cf_bc(to_dfab(phi_fine_fab), fine_lo, fine_hi, to_dfab(crse_old_fab), to_dfab(crse_new_fab), a, (hipStream_t)stream,
                            &c->prof);
}

// ---- Poisson gravity on a refined level of several boxes: one array over their bounding box (poisson_kernels.hip, MgBoxes) -----
int castro_amd_poisson_boxes_plan_create(castro_amd_ctx* c, const double dx[3], int nboxes, const int* lo, const int* hi,
                                         castro_amd_poisson_plan** plan)
{
    if (!c || !plan || !dx || nboxes < 1 || !lo || !hi) return CASTRO_AMD_ERR_ARG;
    // the level table first: a refusal costs no device memory (and needs no device)
    std::vector<MgLevel> lev;
    const int rl = poisson_boxes_levels(nboxes, lo, hi, dx, lev);
    if (rl != 0) return rl;
    hipSetDevice(c->device);
    PoissonPlan* P = nullptr;
    const int rc = poisson_boxes_plan_make(nboxes, lo, hi, dx, &P);
    if (rc != 0) return rc;
    *plan = reinterpret_cast<castro_amd_poisson_plan*>(P);
    return CASTRO_AMD_OK;
}

// the plan of a union of boxes, or nullptr
static PoissonPlan* boxes_plan(castro_amd_poisson_plan* plan)
{
    PoissonPlan* P = reinterpret_cast<PoissonPlan*>(plan);
    return P && !P->flags.empty() ? P : nullptr;
}

// does `f` hold the face values of level L: 3 components on the box with its high corner grown by one?
static bool mgb_faces_ok(const castro_amd_fab* f, const MgLevel& L)
{
    if (!f || !f->p || f->ncomp != 3) return false;
    int hi[3];
    for (int d = 0; d < 3; ++d) hi[d] = L.lo[d] + L.n[d];
    return fab_contains(f, L.lo, hi);
}

// the FABs of the boxes of the plan, each with `ncomp` components (0: at least comp + 1) around its own box
static bool mgb_box_fabs(const PoissonPlan* P, int nboxes, const castro_amd_fab* fabs, int ncomp, int comp, std::vector<DFab>& out)
{
    if (!fabs || nboxes < 1 || (size_t)nboxes != P->boxes.size() / 6) return false;
    out.resize((size_t)nboxes);
    for (int b = 0; b < nboxes; ++b) {
        const castro_amd_fab* f = fabs + b;
        if (!f->p || (ncomp > 0 ? f->ncomp != ncomp : (comp < 0 || comp >= f->ncomp))) return false;
        if (!fab_contains(f, &P->boxes[(size_t)(6 * b)], &P->boxes[(size_t)(6 * b + 3)])) return false;
        out[(size_t)b] = to_dfab(f);
    }
    return true;
}

int castro_amd_poisson_boxes_cf_bc(castro_amd_ctx* c, castro_amd_poisson_plan* plan, const castro_amd_fab* faces_fab,
                                   const castro_amd_fab* crse_old_fab, const castro_amd_fab* crse_new_fab, double a, void* stream)
{
    PoissonPlan* P = boxes_plan(plan);
    if (!c || !P || !(a - a == 0.0) || !mgb_faces_ok(faces_fab, P->lev[0])) return CASTRO_AMD_ERR_ARG;
    const MgLevel& L = P->lev[0];
    int clo[3], chi[3];
    for (int d = 0; d < 3; ++d) { clo[d] = (L.lo[d] >> 1) - 1; chi[d] = ((L.lo[d] + L.n[d] - 1) >> 1) + 1; }
    for (const castro_amd_fab* f : { crse_old_fab, crse_new_fab })
        if (!f || !f->p || f->ncomp != 1 || !fab_contains(f, clo, chi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_phi_cf_boxes(P, to_dfab(faces_fab), to_dfab(crse_old_fab), to_dfab(crse_new_fab), a, (hipStream_t)stream, &c->prof);
}

int castro_amd_poisson_boxes_solve(castro_amd_ctx* c, castro_amd_poisson_plan* plan, const castro_amd_fab* phi_fab,
                                   const castro_amd_fab* faces_fab, int nboxes, const castro_amd_fab* rho_fabs, int rho_comp,
                                   double fourpiG, double reltol, double abstol, int maxiter, int* cycles, int* converged,
                                   double* final_norm, double* h_history, void* stream)
{
    PoissonPlan* P = boxes_plan(plan);
    if (!c || !P || !cycles || !converged || !final_norm || maxiter < 0) return CASTRO_AMD_ERR_ARG;
    const MgLevel& L0 = P->lev[0];
    if (!mg_fab_ok(phi_fab, L0, 1) || phi_fab->ncomp != 1 || !mgb_faces_ok(faces_fab, L0)) return CASTRO_AMD_ERR_ARG;
    std::vector<DFab> U;
    if (!mgb_box_fabs(P, nboxes, rho_fabs, 0, rho_comp, U)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_poisson_boxes_solve(P, to_dfab(phi_fab), to_dfab(faces_fab), U.data(), rho_comp, fourpiG, reltol, abstol, maxiter,
                                      cycles, converged, final_norm, h_history, (hipStream_t)stream, &c->prof);
}

int castro_amd_grad_phi_to_grav_boxes(castro_amd_ctx* c, castro_amd_poisson_plan* plan, const castro_amd_fab* phi_fab,
                                      const castro_amd_fab* faces_fab, int nboxes, const castro_amd_fab* grav_fabs, void* stream)
{
    PoissonPlan* P = boxes_plan(plan);
    if (!c || !P) return CASTRO_AMD_ERR_ARG;
    const MgLevel& L0 = P->lev[0];
    if (!mg_fab_ok(phi_fab, L0, 1) || phi_fab->ncomp != 1 || !mgb_faces_ok(faces_fab, L0)) return CASTRO_AMD_ERR_ARG;
    std::vector<DFab> G;
    if (!mgb_box_fabs(P, nboxes, grav_fabs, 3, 0, G)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_grad_phi_boxes(P, to_dfab(phi_fab), to_dfab(faces_fab), G.data(), (hipStream_t)stream, &c->prof);
}

int castro_amd_poisson_boxes_level_op(castro_amd_ctx* c, castro_amd_poisson_plan* plan, int op, int level, int colour,
                                      const castro_amd_fab* a, const castro_amd_fab* b, const castro_amd_fab* f3,
                                      const castro_amd_fab* faces_fab, double* d_out, void* stream)
{
    PoissonPlan* P = boxes_plan(plan);
    if (!c || !P) return CASTRO_AMD_ERR_ARG;
    const int nl = (int)P->lev.size();
    if (level < 0 || level >= nl) return CASTRO_AMD_ERR_ARG;
    // face values belong to level 0 alone; without them (and on every coarser level) a flagged face holds 0.0
    MgEdge e;
    std::memset(&e, 0, sizeof(e));
    e.flags = P->flags[(size_t)level];
    if (faces_fab) {
        if (level != 0 || !mgb_faces_ok(faces_fab, P->lev[0])) return CASTRO_AMD_ERR_ARG;
        e.X = to_dfab(faces_fab);
    }
    return mg_level_op(c, P, op, level, colour, a, b, f3, e, level + 1 < nl ? P->flags[(size_t)level + 1] : nullptr, d_out, stream);
}

// a gravity FAB of the _gfab source calls: 3 components, one ghost zone around [lo, hi] where the energy term reads neighbours
static bool grav_fab_ok(const castro_amd_fab* g, const int lo[3], const int hi[3], int grav_source_type)
{
    if (!g || !g->p || g->ncomp != 3) return false;
    const int ng = grav_source_type == 4 ? 1 : 0;
    const int glo[3] = { lo[0] - ng, lo[1] - ng, lo[2] - ng }, ghi[3] = { hi[0] + ng, hi[1] + ng, hi[2] + ng };
    return fab_contains(g, glo, ghi);
}

int castro_amd_old_gravity_source_gfab(castro_amd_ctx* c, const castro_amd_fab* state, const castro_amd_fab* source,
                                       const int lo[3], const int hi[3], const castro_amd_fab* grav_old, int grav_source_type,
                                       double dt, void* stream)
{
    if (!c || !state || !state->p || !source || !source->p) return CASTRO_AMD_ERR_ARG;
    if (state->ncomp != NUM_STATE || source->ncomp < 7 || grav_source_type < 1 || grav_source_type > 4) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state, lo, hi) || !fab_contains(source, lo, hi) || !grav_fab_ok(grav_old, lo, hi, 1)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_old_grav_source_gfab(to_dfab(state), to_dfab(source), lo, hi, to_dfab(grav_old), grav_source_type, dt,
                                       (hipStream_t)stream, &c->prof);
}

int castro_amd_new_gravity_source_gfab(castro_amd_ctx* c, const castro_amd_fab* state_old, const castro_amd_fab* state_new,
                                       const castro_amd_fab* source, const castro_amd_fab mass_fluxes[3],
                                       const int lo[3], const int hi[3], const castro_amd_fab* grav_old,
                                       const castro_amd_fab* grav_new, int grav_source_type,
                                       double dt, const castro_amd_geom* geom, void* stream)
{
    if (!c || !state_old || !state_old->p || !state_new || !state_new->p || !source || !source->p || !mass_fluxes || !geom)
        return CASTRO_AMD_ERR_ARG;
    if (state_old->ncomp != NUM_STATE || state_new->ncomp != NUM_STATE || source->ncomp < 7) return CASTRO_AMD_ERR_ARG;
    if (grav_source_type < 1 || grav_source_type > 4 || geom->coord != 0) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state_old, lo, hi) || !fab_contains(state_new, lo, hi) || !fab_contains(source, lo, hi)) return CASTRO_AMD_ERR_ARG;
    if (!grav_fab_ok(grav_old, lo, hi, grav_source_type) || !grav_fab_ok(grav_new, lo, hi, grav_source_type)) return CASTRO_AMD_ERR_ARG;
    DFab M[3];
    if (!mass_flux_dfabs(mass_fluxes, lo, hi, M)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_new_grav_source_gfab(to_dfab(state_old), to_dfab(state_new), to_dfab(source), M, lo, hi, to_dfab(grav_old),
                                       to_dfab(grav_new), grav_source_type, dt, geom->dx, (hipStream_t)stream, &c->prof);
}

// ---- the central point mass (pointmass_kernels.hip) -----------------------------------------------------------------------------
static int pm_geom(const castro_amd_pointmass_params* pm, const castro_amd_geom* geom, PmGeom& G)
{
    if (!pm || !geom) return CASTRO_AMD_ERR_ARG;
    if (geom->coord != 0) return CASTRO_AMD_ERR_UNSUPPORTED;
    for (int d = 0; d < 3; ++d) {
        if (!(geom->dx[d] > 0.0)) return CASTRO_AMD_ERR_ARG;
        G.dx[d] = geom->dx[d]; G.problo[d] = geom->problo[d]; G.center[d] = pm->center[d];
    }
    G.Gconst = pm->Gconst;
    return CASTRO_AMD_OK;
}

int castro_amd_add_pointmass_mf(castro_amd_ctx* c, int nfabs, const castro_amd_fab* grav_fabs, const castro_amd_pointmass_params* pm,
                                const castro_amd_geom* geom, const double* d_point_mass, void* stream)
{
    if (!c || nfabs < 0 || (nfabs > 0 && !grav_fabs) || !d_point_mass) return CASTRO_AMD_ERR_ARG;
    PmGeom G;
    const int rg = pm_geom(pm, geom, G);
    if (rg != CASTRO_AMD_OK) return rg;
    // compared byte by byte with the tables already on the device: every byte is set here
    std::vector<PmFabDev> tab((size_t)nfabs);
    if (nfabs > 0) std::memset((void*)tab.data(), 0, (size_t)nfabs * sizeof(PmFabDev));
    for (int i = 0; i < nfabs; ++i) {
        const castro_amd_fab& f = grav_fabs[i];
        if (!f.p || f.ncomp != 3) return CASTRO_AMD_ERR_ARG;
        const DFab F = to_dfab(&f);
        PmFabDev& T = tab[(size_t)i];
        T.F.p = F.p; T.F.sy = F.sy; T.F.sz = F.sz; T.F.sn = F.sn;
        for (int d = 0; d < 3; ++d) {
            if (f.hi[d] < f.lo[d]) return CASTRO_AMD_ERR_ARG;
            T.F.lo[d] = F.lo[d]; T.lo[d] = f.lo[d]; T.n[d] = f.hi[d] - f.lo[d] + 1;
        }
    }
    hipSetDevice(c->device);
    return launch_add_pointmass(nfabs, tab.data(), G, d_point_mass, &c->pm_tables, (hipStream_t)stream, &c->prof);
}

int castro_amd_add_pointmass_fab(castro_amd_ctx* c, const castro_amd_fab* grav_fab, const castro_amd_pointmass_params* pm,
                                 const castro_amd_geom* geom, const double* d_point_mass, void* stream)
{
    if (!grav_fab) return CASTRO_AMD_ERR_ARG;
    return castro_amd_add_pointmass_mf(c, 1, grav_fab, pm, geom, d_point_mass, stream);
}

// the checks of the two halves of pointmass_update on their box table, the table the kernels read and the cube's low corner
static int pm_boxes(int nboxes, const castro_amd_pointmass_box* boxes, const castro_amd_pointmass_params* pm,
                    const castro_amd_geom* geom, std::vector<PmBoxDev>& tab, int clo[3])
{
    if (nboxes < 0 || (nboxes > 0 && !boxes)) return CASTRO_AMD_ERR_ARG;
    PmGeom G;
    const int rg = pm_geom(pm, geom, G);
    if (rg != CASTRO_AMD_OK) return rg;
    for (int d = 0; d < 3; ++d) {
        // the zone whose lower left corner is at the centre (Castro_pointmass.cpp:38-52); box_size = 2
        const double q = std::floor((pm->center[d] - geom->problo[d]) / geom->dx[d] + 1.e-8);
        if (!(std::fabs(q) < 1.0e9)) return CASTRO_AMD_ERR_ARG;
        clo[d] = (int)q - 2;
    }
    tab.resize((size_t)nboxes);
    if (nboxes > 0) std::memset((void*)tab.data(), 0, (size_t)nboxes * sizeof(PmBoxDev));
    for (int i = 0; i < nboxes; ++i) {
        const castro_amd_pointmass_box& b = boxes[i];
        if (!b.state_old.p || b.state_old.ncomp != NUM_STATE || !fab_contains(&b.state_old, b.lo, b.hi)) return CASTRO_AMD_ERR_ARG;
        if (!b.state_new.p || b.state_new.ncomp != NUM_STATE || !fab_contains(&b.state_new, b.lo, b.hi)) return CASTRO_AMD_ERR_ARG;
        const DFab So = to_dfab(&b.state_old), Sn = to_dfab(&b.state_new);
        PmBoxDev& T = tab[(size_t)i];
        T.So.p = So.p; T.So.sy = So.sy; T.So.sz = So.sz; T.So.sn = So.sn;
        T.Sn.p = Sn.p; T.Sn.sy = Sn.sy; T.Sn.sz = Sn.sz; T.Sn.sn = Sn.sn;
        for (int d = 0; d < 3; ++d) { T.So.lo[d] = So.lo[d]; T.Sn.lo[d] = Sn.lo[d]; T.lo[d] = b.lo[d]; T.hi[d] = b.hi[d]; }
    }
    return CASTRO_AMD_OK;
}

int castro_amd_pointmass_delta_mf(castro_amd_ctx* c, int nboxes, const castro_amd_pointmass_box* boxes,
                                  const castro_amd_pointmass_params* pm, const castro_amd_geom* geom, double* d_delta, void* stream)
{
    if (!c || !d_delta) return CASTRO_AMD_ERR_ARG;
    std::vector<PmBoxDev> tab;
    int clo[3];
    const int rt = pm_boxes(nboxes, boxes, pm, geom, tab, clo);
    if (rt != CASTRO_AMD_OK) return rt;
    hipSetDevice(c->device);
    return launch_pointmass_delta(nboxes, tab.data(), clo, geom->dx[0] * geom->dx[1] * geom->dx[2], d_delta, &c->pm_tables,
                                  (hipStream_t)stream, &c->prof);
}

int castro_amd_pointmass_apply_mf(castro_amd_ctx* c, int nboxes, const castro_amd_pointmass_box* boxes,
                                  const castro_amd_pointmass_params* pm, const castro_amd_geom* geom, const double* d_delta,
                                  double* d_point_mass, void* stream)
{
    if (!c || !d_delta || !d_point_mass) return CASTRO_AMD_ERR_ARG;
    std::vector<PmBoxDev> tab;
    int clo[3];
    const int rt = pm_boxes(nboxes, boxes, pm, geom, tab, clo);
    if (rt != CASTRO_AMD_OK) return rt;
    hipSetDevice(c->device);
    return launch_pointmass_apply(nboxes, tab.data(), clo, d_delta, d_point_mass, &c->pm_tables, (hipStream_t)stream, &c->prof);
}

// ---- tracer particles (tracer_kernels.hip) ---------------------------------------------------------------------------------------
static bool tr_particles_ok(const castro_amd_tracers* t)
{
    if (!t || t->n < 0) return false;
    if (t->n == 0) return true;
    return t->x && t->y && t->z && t->r0 && t->r1 && t->r2 && t->id && t->level && t->grid;
}

// the geometry every tracer kernel reads: problo / probhi, the periodic directions, 1 / dx of the level into dxi[slot]
static int tr_geom(const castro_amd_geom* geom, int slot, TrGeom& G)
{
    if (!geom) return CASTRO_AMD_ERR_ARG;
    if (geom->coord != 0) return CASTRO_AMD_ERR_UNSUPPORTED;
    for (int d = 0; d < 3; ++d) {
        if (!(geom->dx[d] > 0.0) || !(geom->probhi[d] > geom->problo[d])) return CASTRO_AMD_ERR_ARG;
        G.plo[d] = geom->problo[d]; G.phi[d] = geom->probhi[d];
        G.periodic[d] = (geom->lo_bc[d] == 0 && geom->hi_bc[d] == 0) ? 1 : 0;
        G.dxi[slot][d] = 1.0 / geom->dx[d];
    }
    return CASTRO_AMD_OK;
}

// table entries [at, at + nboxes) from the caller's boxes; need_fab: a FAB of at least min_ncomp components that holds the valid
// box -- or none at all (fab.p == NULL: a box of another rank, whose entry keeps a null FAB the kernels skip)
static int tr_boxes(int nboxes, const castro_amd_tracer_box* boxes, bool need_fab, int min_ncomp, std::vector<TrBoxDev>& tab, size_t at)
{
    for (int i = 0; i < nboxes; ++i) {
        const castro_amd_tracer_box& b = boxes[i];
        TrBoxDev& T = tab[at + (size_t)i];
        for (int d = 0; d < 3; ++d) {
            if (b.vhi[d] < b.vlo[d]) return CASTRO_AMD_ERR_ARG;
            T.vlo[d] = b.vlo[d]; T.vhi[d] = b.vhi[d];
        }
        if (need_fab && b.fab.p) {
            if (b.fab.ncomp < min_ncomp || !fab_contains(&b.fab, b.vlo, b.vhi)) return CASTRO_AMD_ERR_ARG;
            const DFab F = to_dfab(&b.fab);
            T.F.p = F.p; T.F.sy = F.sy; T.F.sz = F.sz; T.F.sn = F.sn;
            for (int d = 0; d < 3; ++d) { T.F.lo[d] = F.lo[d]; T.alo[d] = b.fab.lo[d]; T.ahi[d] = b.fab.hi[d]; }
        }
    }
    return CASTRO_AMD_OK;
}

static void tr_zero(std::vector<TrBoxDev>& tab, TrGeom& G)
{
    if (!tab.empty()) std::memset((void*)tab.data(), 0, tab.size() * sizeof(TrBoxDev));
    std::memset((void*)&G, 0, sizeof(TrGeom));
}

int castro_amd_tracer_advect_mf(castro_amd_ctx* c, int level, int nboxes, const castro_amd_tracer_box* boxes,
                                const castro_amd_geom* geom, double dt, int ipass, const castro_amd_tracers* tracers, int* d_flags,
                                void* stream)
{
    if (!c || level < 0 || nboxes < 0 || (nboxes > 0 && !boxes) || !tr_particles_ok(tracers) || !d_flags || (ipass != 0 && ipass != 1))
        return CASTRO_AMD_ERR_ARG;
    std::vector<TrBoxDev> tab((size_t)nboxes);
    TrGeom G;
    tr_zero(tab, G);
    int rt = tr_geom(geom, 0, G);
    if (rt != CASTRO_AMD_OK) return rt;
    rt = tr_boxes(nboxes, boxes, true, UMZ + 1, tab, 0);
    if (rt != CASTRO_AMD_OK) return rt;
    hipSetDevice(c->device);
    return launch_tracer_advect(nboxes, tab.data(), level, G, dt, ipass, *tracers, d_flags, &c->tr_tables, (hipStream_t)stream, &c->prof);
}

int castro_amd_tracer_sample_mf(castro_amd_ctx* c, int level, int nboxes, const castro_amd_tracer_box* boxes,
                                const castro_amd_geom* geom, int ncomps, const int* comps, const castro_amd_tracers* tracers,
                                double* d_out, int* d_flags, void* stream)
{
    if (!c || level < 0 || nboxes < 0 || (nboxes > 0 && !boxes) || !tr_particles_ok(tracers) || !d_flags || !comps || ncomps < 1
        || ncomps > CASTRO_AMD_NUM_STATE || (tracers->n > 0 && !d_out))
        return CASTRO_AMD_ERR_ARG;
    std::vector<TrBoxDev> tab((size_t)nboxes);
    TrGeom G;
    tr_zero(tab, G);
    int rt = tr_geom(geom, 0, G);
    if (rt != CASTRO_AMD_OK) return rt;
    TrComps C;
    std::memset((void*)&C, 0, sizeof(C));
    C.n = ncomps;
    int maxc = 0;
    for (int q = 0; q < ncomps; ++q) {
        if (comps[q] < 0) return CASTRO_AMD_ERR_ARG;
        C.comp[q] = comps[q];
        if (comps[q] > maxc) maxc = comps[q];
    }
    rt = tr_boxes(nboxes, boxes, true, maxc + 1, tab, 0);
    if (rt != CASTRO_AMD_OK) return rt;
    hipSetDevice(c->device);
    return launch_tracer_sample(nboxes, tab.data(), level, G, C, *tracers, d_out, d_flags, &c->tr_tables, (hipStream_t)stream, &c->prof);
}

int castro_amd_tracer_locate(castro_amd_ctx* c, int lev_min, int lev_max, int ngrow, int nlev, const int* nboxes_per_level,
                             const castro_amd_tracer_box* boxes, const castro_amd_geom* geoms, const castro_amd_tracers* tracers,
                             int* d_flags, void* stream)
{
    if (!c || nlev < 1 || nlev > CAD_TRACER_MAX_LEVELS || lev_min < 0 || lev_max < lev_min || lev_max >= nlev || ngrow < 0
        || !nboxes_per_level || !geoms || !tr_particles_ok(tracers) || !d_flags)
        return CASTRO_AMD_ERR_ARG;
    long tot = 0;
    for (int l = 0; l < nlev; ++l) {
        if (nboxes_per_level[l] < 0) return CASTRO_AMD_ERR_ARG;
        tot += nboxes_per_level[l];
    }
    if (tot > 0x7fffffffL || (tot > 0 && !boxes)) return CASTRO_AMD_ERR_ARG;
    std::vector<TrBoxDev> tab((size_t)tot);
    TrGeom G;
    tr_zero(tab, G);
    G.nlev = nlev;
    size_t at = 0;
    for (int l = 0; l < nlev; ++l) {
        TrGeom Gl;
        std::memset((void*)&Gl, 0, sizeof(Gl));
        const int rg = tr_geom(&geoms[l], 0, Gl);
        if (rg != CASTRO_AMD_OK) return rg;
        for (int d = 0; d < 3; ++d) {
            if (l == 0) { G.plo[d] = Gl.plo[d]; G.phi[d] = Gl.phi[d]; G.periodic[d] = Gl.periodic[d]; }
            else if (G.plo[d] != Gl.plo[d] || G.phi[d] != Gl.phi[d] || G.periodic[d] != Gl.periodic[d]) return CASTRO_AMD_ERR_ARG;
            G.dxi[l][d] = Gl.dxi[0][d];
        }
        G.start[l] = (int)at;
        const int rt = tr_boxes(nboxes_per_level[l], boxes + at, false, 0, tab, at);
        if (rt != CASTRO_AMD_OK) return rt;
        at += (size_t)nboxes_per_level[l];
    }
    for (int l = nlev; l <= CAD_TRACER_MAX_LEVELS; ++l) G.start[l] = (int)at;
    hipSetDevice(c->device);
    return launch_tracer_locate((int)tot, tab.data(), G, lev_min, lev_max, ngrow, *tracers, d_flags, &c->tr_tables, (hipStream_t)stream,
                                &c->prof);
}

int castro_amd_tracer_count_mf(castro_amd_ctx* c, int level, int nboxes, const castro_amd_tracer_box* count_boxes,
                               const castro_amd_geom* geom, const castro_amd_tracers* tracers, void* stream)
{
    if (!c || level < 0 || nboxes < 0 || (nboxes > 0 && !count_boxes) || !tr_particles_ok(tracers)) return CASTRO_AMD_ERR_ARG;
    std::vector<TrBoxDev> tab((size_t)nboxes);
    TrGeom G;
    tr_zero(tab, G);
    int rt = tr_geom(geom, 0, G);
    if (rt != CASTRO_AMD_OK) return rt;
    for (int i = 0; i < nboxes; ++i) if (count_boxes[i].fab.p && count_boxes[i].fab.ncomp != 1) return CASTRO_AMD_ERR_ARG;
    rt = tr_boxes(nboxes, count_boxes, true, 1, tab, 0);
    if (rt != CASTRO_AMD_OK) return rt;
    hipSetDevice(c->device);
    return launch_tracer_count(nboxes, tab.data(), level, G, *tracers, &c->tr_tables, (hipStream_t)stream, &c->prof);
}

int castro_amd_tracer_migrate_count(castro_amd_ctx* c, int nlev, const int* nboxes_per_level, const int* owners, int nranks,
                                    int myrank, const castro_amd_tracers* tracers, int* d_dest, int* d_counts, void* stream)
{
    if (!c || nlev < 1 || nlev > CAD_TRACER_MAX_LEVELS || !nboxes_per_level || nranks < 1 || myrank < 0 || myrank >= nranks
        || !tr_particles_ok(tracers) || !d_counts || (tracers->n > 0 && !d_dest) || tracers->n > 0x7fffffffLL)
        return CASTRO_AMD_ERR_ARG;
    if (nranks > CASTRO_AMD_TRACER_MAX_RANKS) return CASTRO_AMD_ERR_UNSUPPORTED;
    TrOwners O;
    std::memset((void*)&O, 0, sizeof(O));
    O.nlev = nlev;
    long tot = 0;
    for (int l = 0; l < nlev; ++l) {
        if (nboxes_per_level[l] < 0) return CASTRO_AMD_ERR_ARG;
        O.start[l] = (int)tot;
        tot += nboxes_per_level[l];
        if (tot > 0x7fffffffL) return CASTRO_AMD_ERR_ARG;
    }
    for (int l = nlev; l <= CAD_TRACER_MAX_LEVELS; ++l) O.start[l] = (int)tot;
    if (tot > 0 && !owners) return CASTRO_AMD_ERR_ARG;
    for (long i = 0; i < tot; ++i) if (owners[i] < 0 || owners[i] >= nranks) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_tracer_migrate_count(owners, (int)tot, O, nranks, myrank, *tracers, d_dest, d_counts, &c->tr_migrate, &c->tr_tables,
                                       (hipStream_t)stream, &c->prof);
}

int castro_amd_tracer_migrate_pack(castro_amd_ctx* c, int nranks, int myrank, const castro_amd_tracers* tracers_in, const int* d_dest,
                                   const castro_amd_tracers* tracers_out, long long* d_wire, long long nwire, void* stream)
{
    if (!c || nranks < 1 || myrank < 0 || myrank >= nranks || !tr_particles_ok(tracers_in) || !tr_particles_ok(tracers_out) || nwire < 0
        || (nwire > 0 && !d_wire) || ((size_t)d_wire & 15) || (tracers_in->n > 0 && !d_dest))
        return CASTRO_AMD_ERR_ARG;
    if (nranks > CASTRO_AMD_TRACER_MAX_RANKS) return CASTRO_AMD_ERR_UNSUPPORTED;
    if (tracers_in->n > 0 && tracers_out->n > 0) {
        // cpu may be NULL (all zero): a NULL never aliases
        const void* in[10] = { tracers_in->x, tracers_in->y, tracers_in->z, tracers_in->r0, tracers_in->r1, tracers_in->r2,
                               tracers_in->id, tracers_in->cpu, tracers_in->level, tracers_in->grid };
        const void* out[10] = { tracers_out->x, tracers_out->y, tracers_out->z, tracers_out->r0, tracers_out->r1, tracers_out->r2,
                                tracers_out->id, tracers_out->cpu, tracers_out->level, tracers_out->grid };
        for (int i = 0; i < 10; ++i) for (int j = 0; j < 10; ++j) if (in[i] && in[i] == out[j]) return CASTRO_AMD_ERR_ARG;
    }
    hipSetDevice(c->device);
    return launch_tracer_migrate_pack(nranks, myrank, *tracers_in, d_dest, *tracers_out, d_wire, nwire, &c->tr_migrate,
                                      (hipStream_t)stream, &c->prof);
}

int castro_amd_tracer_unpack(castro_amd_ctx* c, const long long* d_wire, long long nrecv, const castro_amd_tracers* tracers_out,
                             long long at, void* stream)
{
    if (!c || nrecv < 0 || at < 0 || !tr_particles_ok(tracers_out) || (nrecv > 0 && !d_wire) || ((size_t)d_wire & 15)
        || at > tracers_out->n || nrecv > tracers_out->n - at)
        return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_tracer_unpack(d_wire, nrecv, *tracers_out, at, (hipStream_t)stream, &c->prof);
}

int castro_amd_saxpy_fab(castro_amd_ctx* c, const castro_amd_fab* dst, double a, const castro_amd_fab* src, int ncomp,
                         const int lo[3], const int hi[3], void* stream)
{
    if (!c || !dst || !dst->p || !src || !src->p || ncomp < 1 || ncomp > dst->ncomp || ncomp > src->ncomp) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(dst, lo, hi) || !fab_contains(src, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_saxpy(to_dfab(dst), to_dfab(src), lo, hi, a, ncomp, (hipStream_t)stream, &c->prof);
}

int castro_amd_apply_source_fab(castro_amd_ctx* c, const castro_amd_fab* dst, const castro_amd_fab* base, double a,
                                const castro_amd_fab* src, int nsrc, const int lo[3], const int hi[3],
                                const castro_amd_params* params, int clean_ntimes, void* stream)
{
    if (!c || !dst || !dst->p || !base || !base->p || !src || !src->p || !params || clean_ntimes < 0) return CASTRO_AMD_ERR_ARG;
    if (dst->ncomp != NUM_STATE || base->ncomp != NUM_STATE || nsrc < 0 || nsrc > NUM_STATE || nsrc > src->ncomp) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(dst, lo, hi) || !fab_contains(base, lo, hi) || !fab_contains(src, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_apply_source(to_dfab(dst), to_dfab(base), to_dfab(src), lo, hi, a, nsrc, to_devparams(params), clean_ntimes,
                               (hipStream_t)stream, &c->prof);
}

static bool fab_ok(const castro_amd_fab* f, int ncomp) { return f && f->p && f->ncomp >= ncomp; }

int castro_amd_cc_interp_fab(castro_amd_ctx* c, const castro_amd_fab* crse, const castro_amd_fab* fine,
                             const int lo[3], const int hi[3], int ncomp, void* stream)
{
    if (!c || ncomp < 1 || !fab_ok(crse, ncomp) || !fab_ok(fine, ncomp) || !fab_contains(fine, lo, hi)) return CASTRO_AMD_ERR_ARG;
    int clo[3], chi[3];
    for (int d = 0; d < 3; ++d) {
        clo[d] = (lo[d] >= 0 ? lo[d] / 2 : -((-lo[d] + 1) / 2)) - 1;
        chi[d] = (hi[d] >= 0 ? hi[d] / 2 : -((-hi[d] + 1) / 2)) + 1;
    }
    if (!fab_contains(crse, clo, chi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_cc_interp(to_dfab(crse), to_dfab(fine), lo, hi, ncomp, (hipStream_t)stream, &c->prof);
}

static int fab_ops_impl(castro_amd_ctx* c, int nops, const castro_amd_fab_op* ops, const castro_amd_params* params, void* stream);

int castro_amd_fab_ops(castro_amd_ctx* c, int nops, const castro_amd_fab_op* ops, void* stream)
{
    return fab_ops_impl(c, nops, ops, nullptr, stream);
}

int castro_amd_fab_ops_p(castro_amd_ctx* c, int nops, const castro_amd_fab_op* ops, const castro_amd_params* params, void* stream)
{
    if (!params) return CASTRO_AMD_ERR_ARG;
    return fab_ops_impl(c, nops, ops, params, stream);
}

static int fab_ops_impl(castro_amd_ctx* c, int nops, const castro_amd_fab_op* ops, const castro_amd_params* params, void* stream)
{
    if (!c || nops < 0 || (nops > 0 && !ops)) return CASTRO_AMD_ERR_ARG;
    if (nops == 0) return CASTRO_AMD_OK;
    std::vector<DFab> D(nops), X(nops), Y(nops);
    std::vector<int> lo(3 * nops), hi(3 * nops), kind(nops), dir(nops), side(nops), ncomp(nops);
    std::vector<double> a(nops), b(nops);
    for (int r = 0; r < nops; ++r) {
        const castro_amd_fab_op& o = ops[r];
        if (o.ncomp < 1 || !fab_ok(&o.dst, o.ncomp) || !fab_ok(&o.src, o.ncomp)) return CASTRO_AMD_ERR_ARG;
        if (o.kind != CASTRO_AMD_OP_REFLUX && !fab_contains(&o.dst, o.lo, o.hi)) return CASTRO_AMD_ERR_ARG;
        switch (o.kind) {
        case CASTRO_AMD_OP_CLEAN:
            if (!params || o.ncomp != NUM_STATE || o.dst.ncomp != NUM_STATE || o.a < 0.0) return CASTRO_AMD_ERR_ARG;
            break;
        case CASTRO_AMD_OP_INTERP_CLEAN: {
            if (!params || o.ncomp != NUM_STATE || o.dst.ncomp != NUM_STATE || o.src.ncomp != NUM_STATE || o.a < 0.0) return CASTRO_AMD_ERR_ARG;
            // the coarse zones under the region, grown by one (the slopes of cell_cons_interp)
            int clo[3], chi[3];
            for (int d = 0; d < 3; ++d) { clo[d] = (o.lo[d] >= 0 ? o.lo[d] / 2 : -((-o.lo[d] + 1) / 2)) - 1; chi[d] = (o.hi[d] >= 0 ? o.hi[d] / 2 : -((-o.hi[d] + 1) / 2)) + 1; }
            if (!fab_contains(&o.src, clo, chi)) return CASTRO_AMD_ERR_ARG;
            break; }
        case CASTRO_AMD_OP_INTERP: {
            if (o.ncomp > NUM_STATE) return CASTRO_AMD_ERR_ARG;
            int clo[3], chi[3];
            for (int d = 0; d < 3; ++d) { clo[d] = (o.lo[d] >= 0 ? o.lo[d] / 2 : -((-o.lo[d] + 1) / 2)) - 1; chi[d] = (o.hi[d] >= 0 ? o.hi[d] / 2 : -((-o.hi[d] + 1) / 2)) + 1; }
            if (!fab_contains(&o.src, clo, chi)) return CASTRO_AMD_ERR_ARG;
            break; }
        case CASTRO_AMD_OP_AVGDOWN: {
            int flo[3], fhi[3];
            for (int d = 0; d < 3; ++d) { flo[d] = 2 * o.lo[d]; fhi[d] = 2 * o.hi[d] + 1; }
            if (!fab_contains(&o.src, flo, fhi)) return CASTRO_AMD_ERR_ARG;
            break; }
        case CASTRO_AMD_OP_REFLUX: {
            if (o.dir < 0 || o.dir > 2 || o.side < 0 || o.side > 1 || !fab_contains(&o.src, o.lo, o.hi)) return CASTRO_AMD_ERR_ARG;
            int zlo[3] = { o.lo[0], o.lo[1], o.lo[2] }, zhi[3] = { o.hi[0], o.hi[1], o.hi[2] };
            if (o.side == 0) { zlo[o.dir] -= 1; zhi[o.dir] -= 1; }
            if (!fab_contains(&o.dst, zlo, zhi)) return CASTRO_AMD_ERR_ARG;
            break; }
        case CASTRO_AMD_OP_FLUXREG_TO_FLUX:
            // src2: the mass-flux FAB (one component) or none (p == NULL)
            if (!fab_contains(&o.src, o.lo, o.hi) || (o.src2.p && (o.src2.ncomp < 1 || !fab_contains(&o.src2, o.lo, o.hi)))) return CASTRO_AMD_ERR_ARG;
            break;
        case CASTRO_AMD_OP_LINCOMB:
            if (!fab_ok(&o.src2, o.ncomp) || !fab_contains(&o.src2, o.lo, o.hi)) return CASTRO_AMD_ERR_ARG;
            /* fall through */
        case CASTRO_AMD_OP_COPY:
        case CASTRO_AMD_OP_FLUXREG_CRSE_INIT:
            if (!fab_contains(&o.src, o.lo, o.hi)) return CASTRO_AMD_ERR_ARG;
            break;
        case CASTRO_AMD_OP_FLUXREG_FINE_ADD: {
            if (o.dir < 0 || o.dir > 2) return CASTRO_AMD_ERR_ARG;
            int flo[3], fhi[3];
            for (int d = 0; d < 3; ++d) { flo[d] = 2 * o.lo[d]; fhi[d] = (d == o.dir) ? 2 * o.hi[d] : 2 * o.hi[d] + 1; }
            if (!fab_contains(&o.src, flo, fhi)) return CASTRO_AMD_ERR_ARG;
            break; }
        default:
            return CASTRO_AMD_ERR_ARG;
        }
        D[r] = to_dfab(&o.dst); X[r] = to_dfab(&o.src);
        Y[r] = (o.kind == CASTRO_AMD_OP_LINCOMB || o.kind == CASTRO_AMD_OP_FLUXREG_TO_FLUX) ? to_dfab(&o.src2) : X[r];
        for (int d = 0; d < 3; ++d) { lo[3 * r + d] = o.lo[d]; hi[3 * r + d] = o.hi[d]; }
        kind[r] = o.kind; dir[r] = o.dir; side[r] = o.side; ncomp[r] = o.ncomp; a[r] = o.a; b[r] = o.b;
    }
    hipSetDevice(c->device);
    DevParams P;
    if (params) P = to_devparams(params);
    return launch_fab_ops(nops, D.data(), X.data(), Y.data(), lo.data(), hi.data(), kind.data(), dir.data(), side.data(), ncomp.data(),
                          a.data(), b.data(), (hipStream_t)stream, &c->prof, params ? &P : nullptr, &c->ops_arena);
}

int castro_amd_ctu_hydro_mf(castro_amd_ctx* const* ctxs, void* const* streams, int nctx,
                            const castro_amd_hydro_box* boxes, int nboxes,
                            const castro_amd_geom* geom, const castro_amd_params* params,
                            double time, double dt, const castro_amd_hydro_opts* opts, void* stream)
{
    if (!ctxs || !streams || nctx < 1 || nboxes < 0 || (nboxes > 0 && !boxes) || !geom || !params || !opts) return CASTRO_AMD_ERR_ARG;
    for (int k = 0; k < nctx; ++k) if (!ctxs[k]) return CASTRO_AMD_ERR_ARG;
    if (nboxes == 0) return CASTRO_AMD_OK;
    hipStream_t main_s = (hipStream_t)stream;
    // The whole level as ONE grid per kernel (default options, no source terms: launch_ctu_hydro_level): every box gets
    // its own scratch inside the first context's arena, the per-box arguments travel in a device table, 8 launches on the
    // caller's stream whatever the number of boxes.  CASTRO_AMD_LEVEL_GRID=0 keeps the per-box launches on nctx streams.
    {
        static const bool level_grid = [] { const char* e = std::getenv("CASTRO_AMD_LEVEL_GRID"); return !e || std::atoi(e) != 0; }();
        bool ok = level_grid && nboxes >= 2;
        // traced source terms (round 6): every box with its source FAB or none; a context that carries a source corrector
        // (castro.source_term_predictor = 1: one per box and context) stays box by box
        const bool with_src = boxes[0].src.p != nullptr;
        for (int i = 0; i < nboxes && ok; ++i) ok = (boxes[i].src.p != nullptr) == with_src;
        if (with_src && (params->source_term_predictor == 1 || ctxs[0]->src_corr.p || opts->sborder_clean_ntimes > 0 || opts->clean_ntimes > 0)) ok = false;
        DevParams devP = to_devparams(params);
        devP.dtp = opts->d_dt;
        if (ok && level_launch_supported(ctxs[0]->knobs, devP, opts->flags, with_src)) {
            castro_amd_ctx* c0 = ctxs[0];
            hipSetDevice(c0->device);
            std::vector<PreparedBox> pb((size_t)nboxes);
            std::vector<size_t> need((size_t)nboxes);
            for (int i = 0; i < nboxes; ++i) {
                const castro_amd_hydro_box& b = boxes[i];
                int rc = prepare_box(c0, b.bxlo, b.bxhi, b.vbxlo, b.vbxhi, &b.Sborder, &b.src, &b.S_new, b.flux, b.mass_flux, b.qe,
                                     geom, params, opts, pb[(size_t)i]);
                if (rc != CASTRO_AMD_OK) return rc;
                need[(size_t)i] = (size_t)pb[(size_t)i].t.NC * (size_t)kPlanes;
            }
            // Scratch of a level-wide launch: kPlanes planes (1.26 KB) per ghosted zone of EVERY box of the launch at once, where
            // the box-by-box path needs the largest box only.  So the level goes out in chunks of consecutive boxes whose scratch
            // fits a byte budget (CASTRO_AMD_LEVEL_SCRATCH_GB, default 32; a single box larger than that is a chunk of its own):
            // 8 launches per chunk, the chunks one after the other on the caller's stream in the same arena.  If the arena cannot
            // be had at all the call falls through to the box-by-box path below, which needs the largest box only.
            const double budget_gb = [] { const char* e = std::getenv("CASTRO_AMD_LEVEL_SCRATCH_GB"); const double v = e ? std::atof(e) : 32.0; return v > 0.0 ? v : 32.0; }();   // read per call: a host may change it between levels
            const size_t budget = (size_t)(budget_gb * 1073741824.0 / sizeof(double));
            std::vector<int> first;                       // first box of every chunk
            size_t cur = 0, largest = 0;
            for (int i = 0; i < nboxes; ++i) {
                if (i == 0 || cur + need[(size_t)i] > budget) {
                    first.push_back(i);
                    cur = 0;
                }
                cur += need[(size_t)i];
                if (cur > largest) largest = cur;
            }
            first.push_back(nboxes);
            bool have_arena = largest <= c0->arena_doubles;
            if (!have_arena) {
                if (c0->arena) { hipDeviceSynchronize(); hipFree(c0->arena); c0->arena = nullptr; c0->arena_doubles = 0; }
                if (hipMalloc(&c0->arena, largest * sizeof(double)) == hipSuccess) { c0->arena_doubles = largest; have_arena = true; }
                else { (void)hipGetLastError(); c0->arena = nullptr; }
            }
            if (have_arena) {
                const DevGeom dg = to_devgeom(geom);
                for (size_t ch = 0; ch + 1 < first.size(); ++ch) {
                    const int i0 = first[ch], i1 = first[ch + 1];
                    if (i1 - i0 == 1 && first.size() > 2) {
                        // a chunk of one box: the ordinary call (its own kernels need no table), same arena, same stream
                        const castro_amd_hydro_box& b = boxes[i0];
                        const int rc = castro_amd_ctu_hydro_fab_ex(c0, b.bxlo, b.bxhi, b.vbxlo, b.vbxhi, &b.Sborder, &b.src, &b.S_new,
                                                                   b.flux, b.mass_flux, b.qe, geom, params, time, dt, opts, main_s);
                        if (rc != CASTRO_AMD_OK) return rc;
                        continue;
                    }
                    std::vector<LevelBoxDesc> lb((size_t)(i1 - i0));
                    double* p = c0->arena;
                    for (int i = i0; i < i1; ++i) {
                        const PreparedBox& B = pb[(size_t)i];
                        LevelBoxDesc& L = lb[(size_t)(i - i0)];
                        L.t = B.t;
                        p = carve_scratch(p, B.t, false, L.S);
                        L.U = B.dS; L.Unew = B.dN; L.Src = B.dSrc;
                        for (int d = 0; d < 3; ++d) { L.fl[d] = B.dF[d]; L.mass[d] = B.dM[d]; L.qe[d] = B.dQ[d]; L.acc_hi[d] = B.acc_hi[d]; }
                    }
                    const int rc = launch_ctu_hydro_level(c0->knobs, i1 - i0, lb.data(), &c0->level_arena, dg, devP, dt, opts->flags, c0->d_status,
                                                          main_s, &c0->prof, opts->clean_ntimes, opts->d_out, opts->sborder_clean_ntimes);
                    if (rc != 0) return rc;
                }
                return CASTRO_AMD_OK;
            }
            // no arena: box by box
        }
    }
    const int used = nboxes < nctx ? nboxes : nctx;
    const bool forked = !(used == 1 && (hipStream_t)streams[0] == main_s);
    castro_amd_ctx* c0 = ctxs[0];
    hipSetDevice(c0->device);
    if (forked) {
        if (!c0->mf_fork && hipEventCreateWithFlags(&c0->mf_fork, hipEventDisableTiming) != hipSuccess) return CASTRO_AMD_ERR_HIP;
        hipEventRecord(c0->mf_fork, main_s);
        for (int k = 0; k < used; ++k)
            if ((hipStream_t)streams[k] != main_s) hipStreamWaitEvent((hipStream_t)streams[k], c0->mf_fork, 0);
    }
    int rc = CASTRO_AMD_OK;
    for (int i = 0; i < nboxes && rc == CASTRO_AMD_OK; ++i) {
        const castro_amd_hydro_box& b = boxes[i];
        rc = castro_amd_ctu_hydro_fab_ex(ctxs[i % nctx], b.bxlo, b.bxhi, b.vbxlo, b.vbxhi, &b.Sborder, &b.src, &b.S_new,
                                         b.flux, b.mass_flux, b.qe, geom, params, time, dt, opts, streams[i % nctx]);
    }
    if (forked) {
        // join even after an error: the caller's stream must not run ahead of launches already made
        for (int k = 0; k < used; ++k) {
            if ((hipStream_t)streams[k] == main_s) continue;
            castro_amd_ctx* ck = ctxs[k];
            if (!ck->mf_join && hipEventCreateWithFlags(&ck->mf_join, hipEventDisableTiming) != hipSuccess) {
                // no event for this stream: join it the slow way (never under capture: the events exist after the first
                // eager call), record the error and keep joining the others
                hipStreamSynchronize((hipStream_t)streams[k]);
                ck->mf_join = nullptr;
                if (rc == CASTRO_AMD_OK) rc = CASTRO_AMD_ERR_HIP;
                continue;
            }
            hipEventRecord(ck->mf_join, (hipStream_t)streams[k]);
            hipStreamWaitEvent(main_s, ck->mf_join, 0);
        }
    }
    return rc;
}

int castro_amd_fillpatch_shell_fab(castro_amd_ctx* c, const castro_amd_fab* crse, const castro_amd_fab* fine,
                                   const int vlo[3], const int vhi[3], int ngrow, const castro_amd_params* params,
                                   int clean_ntimes, void* stream)
{
    if (!c || !params || !fab_ok(crse, NUM_STATE) || !fab_ok(fine, NUM_STATE) || ngrow < 1 || clean_ntimes < 0) return CASTRO_AMD_ERR_ARG;
    if (crse->ncomp != NUM_STATE || fine->ncomp != NUM_STATE) return CASTRO_AMD_ERR_ARG;
    int glo[3], ghi[3], clo[3], chi[3];
    for (int d = 0; d < 3; ++d) {
        if (vhi[d] < vlo[d]) return CASTRO_AMD_ERR_ARG;
        glo[d] = vlo[d] - ngrow; ghi[d] = vhi[d] + ngrow;
        clo[d] = (glo[d] >= 0 ? glo[d] / 2 : -((-glo[d] + 1) / 2)) - 1;
        chi[d] = (ghi[d] >= 0 ? ghi[d] / 2 : -((-ghi[d] + 1) / 2)) + 1;
    }
    if (!fab_contains(fine, glo, ghi) || !fab_contains(crse, clo, chi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_fillpatch_shell(to_dfab(crse), to_dfab(fine), vlo, vhi, ngrow, to_devparams(params), clean_ntimes,
                                  (hipStream_t)stream, &c->prof);
}

int castro_amd_avgdown_fab(castro_amd_ctx* c, const castro_amd_fab* fine, const castro_amd_fab* crse,
                           const int lo[3], const int hi[3], int ncomp, void* stream)
{
    if (!c || ncomp < 1 || !fab_ok(crse, ncomp) || !fab_ok(fine, ncomp) || !fab_contains(crse, lo, hi)) return CASTRO_AMD_ERR_ARG;
    int flo[3], fhi[3];
    for (int d = 0; d < 3; ++d) { flo[d] = 2 * lo[d]; fhi[d] = 2 * hi[d] + 1; }
    if (!fab_contains(fine, flo, fhi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_avgdown(to_dfab(fine), to_dfab(crse), lo, hi, ncomp, (hipStream_t)stream, &c->prof);
}

int castro_amd_fluxreg_crse_init_fab(castro_amd_ctx* c, const castro_amd_fab* reg, const castro_amd_fab* crse_flux,
                                     const int lo[3], const int hi[3], int ncomp, double mult, void* stream)
{
    if (!c || ncomp < 1 || !fab_ok(reg, ncomp) || !fab_ok(crse_flux, ncomp)) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(reg, lo, hi) || !fab_contains(crse_flux, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_fluxreg(to_dfab(reg), to_dfab(crse_flux), lo, hi, 0, ncomp, mult, 0, (hipStream_t)stream, &c->prof);
}

int castro_amd_fluxreg_fine_add_fab(castro_amd_ctx* c, const castro_amd_fab* reg, const castro_amd_fab* fine_flux,
                                    const int lo[3], const int hi[3], int dir, int ncomp, double mult, void* stream)
{
    if (!c || ncomp < 1 || dir < 0 || dir > 2 || !fab_ok(reg, ncomp) || !fab_ok(fine_flux, ncomp) || !fab_contains(reg, lo, hi))
        return CASTRO_AMD_ERR_ARG;
    int flo[3], fhi[3];
    for (int d = 0; d < 3; ++d) { flo[d] = 2 * lo[d]; fhi[d] = (d == dir) ? 2 * hi[d] : 2 * hi[d] + 1; }
    if (!fab_contains(fine_flux, flo, fhi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_fluxreg(to_dfab(reg), to_dfab(fine_flux), lo, hi, dir, ncomp, mult, 1, (hipStream_t)stream, &c->prof);
}

int castro_amd_fluxreg_to_flux_fab(castro_amd_ctx* c, const castro_amd_fab* flux, const castro_amd_fab* reg,
                                   const castro_amd_fab* mass_flux, const int lo[3], const int hi[3], int ncomp, void* stream)
{
    if (!c || !lo || !hi || ncomp < 1 || !fab_ok(flux, ncomp) || !fab_ok(reg, ncomp)) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(flux, lo, hi) || !fab_contains(reg, lo, hi)) return CASTRO_AMD_ERR_ARG;
    const bool mass = mass_flux && mass_flux->p;
    if (mass && (mass_flux->ncomp < 1 || !fab_contains(mass_flux, lo, hi))) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_fluxreg_to_flux(to_dfab(flux), to_dfab(reg), to_dfab(mass ? mass_flux : nullptr), lo, hi, ncomp,
                                  (hipStream_t)stream, &c->prof);
}

int castro_amd_reflux_fab(castro_amd_ctx* c, const castro_amd_fab* state, const castro_amd_fab* reg,
                          const int lo[3], const int hi[3], int dir, int side, int ncomp, double vol, void* stream)
{
    if (!c || ncomp < 1 || dir < 0 || dir > 2 || side < 0 || side > 1 || !fab_ok(reg, ncomp) || !fab_ok(state, ncomp)) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(reg, lo, hi)) return CASTRO_AMD_ERR_ARG;
    int zlo[3] = { lo[0], lo[1], lo[2] }, zhi[3] = { hi[0], hi[1], hi[2] };
    if (side == 0) { zlo[dir] -= 1; zhi[dir] -= 1; }
    if (!fab_contains(state, zlo, zhi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_reflux(to_dfab(state), to_dfab(reg), lo, hi, dir, side, ncomp, vol, (hipStream_t)stream, &c->prof);
}

int castro_amd_error_tag_fab(castro_amd_ctx* c, const castro_amd_fab* field, int comp, const castro_amd_fab* tags,
                             const int lo[3], const int hi[3], int kind, double value, void* stream)
{
    if (!c || !field || !field->p || !tags || !tags->p || comp < 0 || comp >= field->ncomp || kind < 0 || kind > 3) return CASTRO_AMD_ERR_ARG;
    int glo[3], ghi[3];
    const int g1 = kind >= 2 ? 1 : 0;
    for (int d = 0; d < 3; ++d) { glo[d] = lo[d] - g1; ghi[d] = hi[d] + g1; }
    if (!fab_contains(field, glo, ghi) || !fab_contains(tags, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_error_tag(to_dfab(field), comp, to_dfab(tags), lo, hi, kind, value, (hipStream_t)stream, &c->prof);
}

int castro_amd_lincomb_fab(castro_amd_ctx* c, const castro_amd_fab* dst, double a, const castro_amd_fab* x, double b,
                           const castro_amd_fab* y, int ncomp, const int lo[3], const int hi[3], void* stream)
{
    if (!c || ncomp < 1 || !fab_ok(dst, ncomp) || !fab_ok(x, ncomp) || !fab_ok(y, ncomp)) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(dst, lo, hi) || !fab_contains(x, lo, hi) || !fab_contains(y, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_lincomb(to_dfab(dst), to_dfab(x), to_dfab(y), lo, hi, a, b, ncomp, (hipStream_t)stream, &c->prof);
}

int castro_amd_derive_fab(castro_amd_ctx* c, int which, const castro_amd_fab* state, const castro_amd_fab* der, int dcomp,
                          const int lo[3], const int hi[3], const castro_amd_geom* geom, const castro_amd_params* params,
                          const double center[3], void* stream)
{
    if (!c || !state || !state->p || !der || !der->p || !geom || !params || !center) return CASTRO_AMD_ERR_ARG;
    if (which < 0 || which >= CASTRO_AMD_DER_COUNT || state->ncomp != NUM_STATE) return CASTRO_AMD_ERR_ARG;
    if (dcomp < 0 || dcomp >= der->ncomp || !fab_contains(der, lo, hi)) return CASTRO_AMD_ERR_ARG;
    if (geom->coord != 0) return CASTRO_AMD_ERR_UNSUPPORTED;
    int slo[3], shi[3];
    const int g1 = (which == CASTRO_AMD_DER_MAGVORT || which == CASTRO_AMD_DER_DIVU) ? 1 : 0;   // grow_box_by_one
    for (int d = 0; d < 3; ++d) { slo[d] = lo[d] - g1; shi[d] = hi[d] + g1; }
    if (!fab_contains(state, slo, shi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_derive(which, to_dfab(state), to_dfab(der), dcomp, lo, hi, geom->dx, geom->problo,
                         to_devparams(params), center, (hipStream_t)stream, &c->prof);
}

int castro_amd_bc_fill_fab(castro_amd_ctx* c, const castro_amd_fab* state, const castro_amd_geom* geom, void* stream)
{
    if (!c || !state || !state->p || !geom) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_bc_fill(to_dfab(state), state->lo, state->hi, state->ncomp, to_devgeom(geom),
                          geom->lo_bc, geom->hi_bc, (hipStream_t)stream, &c->prof);
}

int castro_amd_ext_bc_fill_fab(castro_amd_ctx* c, const castro_amd_fab* state, const castro_amd_geom* geom,
                               const castro_amd_params* params, const castro_amd_ext_bc* ext, int* d_unconverged, void* stream)
{
    if (!c || !state || !state->p || !geom || !params || !ext) return CASTRO_AMD_ERR_ARG;
    if (state->ncomp != NUM_STATE) return CASTRO_AMD_OK;          // not the state: a derive's fill ends after the generic part
    hipSetDevice(c->device);
    return launch_ext_bc_fill(to_dfab(state), state->lo, state->hi, geom, to_devparams(params), ext, d_unconverged,
                              (hipStream_t)stream, &c->prof);
}

int castro_amd_copy_fab(castro_amd_ctx* c, const castro_amd_fab* dst, const castro_amd_fab* src,
                        const int lo[3], const int hi[3], void* stream)
{
    if (!c || !dst || !src || !dst->p || !src->p || dst->ncomp != src->ncomp) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(dst, lo, hi) || !fab_contains(src, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_copy(to_dfab(dst), to_dfab(src), lo, hi, src->ncomp, (hipStream_t)stream, &c->prof);
}

int castro_amd_pack_fab(castro_amd_ctx* c, const castro_amd_fab* fab, const int lo[3], const int hi[3],
                        double* buf, void* stream)
{
    if (!c || !fab || !fab->p || !buf || !fab_contains(fab, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_pack(to_dfab(fab), lo, hi, fab->ncomp, buf, 0, (hipStream_t)stream, &c->prof);
}

int castro_amd_unpack_fab(castro_amd_ctx* c, const castro_amd_fab* fab, const int lo[3], const int hi[3],
                          const double* buf, void* stream)
{
    if (!c || !fab || !fab->p || !buf || !fab_contains(fab, lo, hi)) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_pack(to_dfab(fab), lo, hi, fab->ncomp, const_cast<double*>(buf), 1, (hipStream_t)stream, &c->prof);
}

static int pack_regions(castro_amd_ctx* c, const castro_amd_fab* fab, int nregions, const int* lo, const int* hi,
                        const long long* offsets, double* buf, int unpack, void* stream)
{
    if (!c || !fab || !fab->p || !buf || !lo || !hi || !offsets || nregions < 0 || nregions > CASTRO_AMD_MAX_REGIONS)
        return CASTRO_AMD_ERR_ARG;
    for (int r = 0; r < nregions; ++r)
        if (!fab_contains(fab, lo + 3 * r, hi + 3 * r) || offsets[r] < 0) return CASTRO_AMD_ERR_ARG;
    hipSetDevice(c->device);
    return launch_pack_regions(to_dfab(fab), nregions, lo, hi, offsets, fab->ncomp, buf, unpack, (hipStream_t)stream, &c->prof);
}

int castro_amd_pack_regions_fab(castro_amd_ctx* c, const castro_amd_fab* fab, int nregions, const int* lo, const int* hi,
                                const long long* offsets, double* buf, void* stream)
{ return pack_regions(c, fab, nregions, lo, hi, offsets, buf, 0, stream); }

int castro_amd_unpack_regions_fab(castro_amd_ctx* c, const castro_amd_fab* fab, int nregions, const int* lo, const int* hi,
                                  const long long* offsets, const double* buf, void* stream)
{ return pack_regions(c, fab, nregions, lo, hi, offsets, const_cast<double*>(buf), 1, stream); }

// Exec/hydro_tests/Sedov/problem_initialize.H:8-113 (host part) + the per-zone kernel
int castro_amd_sedov_init_fab(castro_amd_ctx* c, const castro_amd_fab* state, const int lo[3], const int hi[3],
                              const castro_amd_geom* geom, const castro_amd_params* params,
                              double r_init, double p_ambient, double exp_energy, double dens_ambient,
                              int nsub, void* stream)
{
    if (!c || !state || !state->p || !geom || !params || state->ncomp != NUM_STATE) return CASTRO_AMD_ERR_ARG;
    if (!fab_contains(state, lo, hi)) return CASTRO_AMD_ERR_ARG;
    double center[3];
    for (int n = 0; n < 3; ++n) center[n] = 0.5 * (geom->problo[n] + geom->probhi[n]);
    // eos(eos_input_rp)
    const double g = params->eos_gamma;
    const double e_ambient = p_ambient / ((g - 1.0) * dens_ambient);
    const double mu = 1.0 / (1.0 * (1.0 / params->abar));          // xn = 1 (problem_initialize.H:25-29)
    const double temp_ambient = (g - 1.0) * e_ambient * (mu * M_U) / K_B;
    const double vctr = (4.0 / 3.0) * M_PI * r_init * r_init * r_init;
    const double e_exp = exp_energy / vctr / dens_ambient;
    hipSetDevice(c->device);
    return launch_sedov_init(to_dfab(state), lo, hi, to_devparams(params), geom->dx, geom->problo, center,
                             r_init, e_exp, e_ambient, temp_ambient, dens_ambient, nsub, (hipStream_t)stream, &c->prof);
}

int castro_amd_sod_init_fab(castro_amd_ctx* c, const castro_amd_fab* state, const int lo[3], const int hi[3],
                            const castro_amd_geom* geom, const castro_amd_params* params,
                            double rho_l, double u_l, double p_l, double rho_r, double u_r, double p_r,
                            int idir, double frac, void* stream)
{
    if (!c || !state || !state->p || !geom || !params || state->ncomp != NUM_STATE) return CASTRO_AMD_ERR_ARG;
    if (idir < 1 || idir > 3 || !fab_contains(state, lo, hi)) return CASTRO_AMD_ERR_ARG;
    const double g = params->eos_gamma;
    const double split = frac * (geom->problo[idir - 1] + geom->probhi[idir - 1]);
    const double e_l = p_l / ((g - 1.0) * rho_l), e_r = p_r / ((g - 1.0) * rho_r);
    const double mu = 1.0 / (1.0 * (1.0 / params->abar));          // xn = 1
    const double T_l = (g - 1.0) * e_l * (mu * M_U) / K_B;
    const double T_r = (g - 1.0) * e_r * (mu * M_U) / K_B;
    hipSetDevice(c->device);
    return launch_sod_init(to_dfab(state), lo, hi, geom->dx, geom->problo, split, idir - 1,
                           rho_l, u_l, rho_l * e_l, T_l, rho_r, u_r, rho_r * e_r, T_r, (hipStream_t)stream, &c->prof);
}

int castro_amd_ctx_set_source_corrector(castro_amd_ctx* c, const castro_amd_fab* corr)
{
    if (!c) return CASTRO_AMD_ERR_ARG;
    if (corr && corr->p) {
        if (corr->ncomp < 7) return CASTRO_AMD_ERR_ARG;
        c->src_corr = *corr;
    } else {
        c->src_corr.p = nullptr;
    }
    return CASTRO_AMD_OK;
}

int castro_amd_ctx_poison_scratch(castro_amd_ctx* c, void* stream)
{
    if (!c) return CASTRO_AMD_ERR_ARG;
    if (!c->arena) return CASTRO_AMD_OK;
    hipSetDevice(c->device);
    // all-ones bytes are a NaN in every double
    return hipMemsetAsync(c->arena, 0xFF, c->arena_doubles * sizeof(double), (hipStream_t)stream) == hipSuccess
        ? CASTRO_AMD_OK : CASTRO_AMD_ERR_HIP;
}

int castro_amd_ctx_profile(castro_amd_ctx* c, int enable)
{
    if (!c) return CASTRO_AMD_ERR_ARG;
    c->prof.enabled = enable != 0;
    return CASTRO_AMD_OK;
}

int castro_amd_ctx_profile_count(castro_amd_ctx* c)
{
    if (!c) return 0;
    prof_collect(&c->prof);
    return (int)c->prof.recs.size();
}

int castro_amd_ctx_profile_get(castro_amd_ctx* c, int idx, char* name, int name_len, double* total_ms, long long* launches)
{
    if (!c || idx < 0 || idx >= (int)c->prof.recs.size()) return CASTRO_AMD_ERR_ARG;
    const auto& r = c->prof.recs[idx];
    if (name && name_len > 0) { std::strncpy(name, r.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    if (total_ms) *total_ms = r.total_ms;
    if (launches) *launches = r.launches;
    return CASTRO_AMD_OK;
}

void castro_amd_ctx_profile_reset(castro_amd_ctx* c)
{
    if (!c) return;
    prof_collect(&c->prof);
    for (auto& r : c->prof.recs) { r.total_ms = 0.0; r.launches = 0; }
}

} // extern "C"

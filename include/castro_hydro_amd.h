/*
 * castro_hydro_amd.h -- C ABI of the MI355X-native CTU hydro path for Castro.
 *
 * Drop-in boundary.  The reference has no FFI for this
 * path: the seam is the C++ member
 *     void Castro::construct_ctu_hydro_source(amrex::Real time, amrex::Real dt)
 *     (Source/hydro/Castro_hydro.H:44, body Source/hydro/Castro_ctu_hydro.cpp:16-1528),
 * called from Castro::do_advance_ctu (Source/driver/Castro_advance_ctu.cpp:156).
 * castro_amd_ctu_hydro_fab() replaces the body of its MFIter loop
 * (Castro_ctu_hydro.cpp:130-1480) for ONE FArrayBox / tile; the other entry
 * points replace the per-FAB sweeps the driver runs either side of it.
 *
 * Conventions
 *  - Arrays are AMReX FArrayBox memory: Fortran order, i fastest, component
 *    slowest, described by (pointer, lo[3], hi[3], ncomp) exactly like the
 *    reference's legacy BL_FORT_FAB_ARG_3D convention
 *    (Source/driver/Castro_F.H:19-34).  All pointers are DEVICE pointers
 *    (hipMalloc / AMReX The_Arena() on a HIP build).  FP64 only.
 *  - State layout is the Sedov build's: NUM_STATE = 8
 *    (URHO UMX UMY UMZ UEDEN UEINT UTEMP UFS), one species.
 *  - The caller owns every array for the duration of the call AND until the
 *    stream is synchronised (the AMReX analogue is Elixir,
 *    Castro_ctu_hydro.cpp:79-82).  The callee owns its scratch (the context).
 *  - Every call is asynchronous on `stream` (a hipStream_t passed as void*;
 *    NULL = the default stream).  No call allocates or synchronises once the
 *    context has been reserved for the tile size.
 *  - Error convention: the reference aborts on CPU and is silent on GPU
 *    (advection_util.cpp:56-68); here every entry point returns an int status
 *    (0 = ok, <0 = bad argument / unsupported option) and never aborts.
 *    Data-dependent failures (rho <= 0 met in ctoprim) are latched in a device
 *    flag readable with castro_amd_ctx_status().
 *  - A context is bound to one device and must be used from one stream at a
 *    time (re-entrant per (device, stream): create one context per stream).
 *  - Thread safety: different host threads may drive different contexts
 *    concurrently (the reference calls the path from inside `#pragma omp
 *    parallel`, Castro_ctu_hydro.cpp:66-72); ONE context must not be entered
 *    by two threads at once.  The CASTRO_AMD_* environment knobs are read by
 *    castro_amd_ctx_create() into the context it returns and apply to that
 *    context only: creating a context changes nothing for the others, so
 *    contexts may be created while other threads are inside calls.
 */
#ifndef CASTRO_HYDRO_AMD_H
#define CASTRO_HYDRO_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header: bumped whenever the meaning or the SIZE of anything a caller allocates changes.
 *   3: reduction vectors (`d_out`) are THREE device doubles (0.2 had two): castro_amd_ctu_hydro_clean_fab,
 *      castro_amd_ctu_hydro_fab_ex / _mf (opts.d_out), castro_amd_clean_state_reduce_fab.
 *   4: castro_amd_numerics(), castro_amd_fill_boundary*(), castro_amd_abi_version().
 *   5: CASTRO_AMD_STAGE_VALID / _REST / CASTRO_AMD_BC_FILL, castro_amd_fill_boundary_ex, castro_amd_halo_plan_wait_packed,
 *      castro_amd_halo_group_* / castro_amd_fill_boundary_group (several boxes per rank), castro_amd_berger_rigoutsos;
 *      castro_amd_hydro_opts.sborder_clean_ntimes is accepted by the staged calls; CASTRO_AMD_OP_INTERP, castro_amd_sources_mf,
 *      castro_amd_clean_state_reduce_mf, castro_amd_estdt_mf.
 *   5 (not bumped: new entry points and a new struct only, nothing an existing caller allocates changes size or meaning):
 *      castro_amd_diffusion, castro_amd_temp_diffusion_fab / _mf, castro_amd_estdt_temp_diffusion_fab / _mf,
 *      castro_amd_sources_mf_ex; castro_amd_integrated_quantities_mf, castro_amd_diag_workgroups (struct castro_amd_diag_box);
 *      castro_amd_radial_mass_mf, castro_amd_radial_gravity, castro_amd_monopole_grav_fab (struct castro_amd_monopole_params),
 *      castro_amd_old_gravity_source_gfab, castro_amd_new_gravity_source_gfab;
 *      castro_amd_new_sponge_source_fab (struct castro_amd_sponge), castro_amd_sources_mf_opts (struct castro_amd_source_opts);
 *      castro_amd_add_pointmass_fab / _mf, castro_amd_pointmass_delta_mf, castro_amd_pointmass_apply_mf (structs
 *      castro_amd_pointmass_params, castro_amd_pointmass_box);
 *      castro_amd_fluxreg_to_flux_fab, CASTRO_AMD_OP_FLUXREG_TO_FLUX, CASTRO_AMD_SOURCES_AFTER_REFLUX (stage 1 | that flag of
 *      castro_amd_sources_mf / _ex / _g / _opts);
 *      castro_amd_tracer_advect_mf, castro_amd_tracer_locate, castro_amd_tracer_sample_mf, castro_amd_tracer_count_mf (structs
 *      castro_amd_tracers, castro_amd_tracer_box);
 *      castro_amd_tracer_migrate_count, castro_amd_tracer_migrate_pack, castro_amd_tracer_unpack
 *      (CASTRO_AMD_TRACER_MAX_RANKS); a castro_amd_tracer_box without a FAB (fab.p == NULL) is accepted by
 *      castro_amd_tracer_advect_mf / _sample_mf / _count_mf, which refused it before.
 *      castro_amd_fab_pack, castro_amd_fab_unpack (struct castro_amd_pack_entry): the valid zones of many FABs into one
 *      contiguous buffer and back, for checkpoints.
 *      castro_amd_multipole_moments_mf, castro_amd_multipole_phi_bc_fab (struct castro_amd_multipole),
 *      castro_amd_poisson_plan_create / _destroy, castro_amd_poisson_solve, castro_amd_poisson_level_op,
 *      castro_amd_grad_phi_to_grav_fab: Poisson self-gravity on a single level.
 *      castro_amd_poisson_cf_bc_fab: the coarse-fine boundary potential of a refined level's own Poisson solve.
 *      castro_amd_poisson_boxes_plan_create, castro_amd_poisson_boxes_cf_bc, castro_amd_poisson_boxes_solve,
 *      castro_amd_grad_phi_to_grav_boxes, castro_amd_poisson_boxes_level_op: the level solve of a refined level of several boxes.
 * A caller checks `castro_amd_abi_version() == CASTRO_AMD_ABI_VERSION` once after loading the library; a mismatch means
 * the library was built from another revision of this header (a 0.2 caller with 2-double vectors would be written 8 bytes
 * out of bounds by a 0.3 library). */
#define CASTRO_AMD_ABI_VERSION 5
/* release of the library: castro_amd_version() is "castro_hydro_amd <this> (gfx950, numerics=...)" -- the one place it is written */
#define CASTRO_AMD_RELEASE "0.6"

#define CASTRO_AMD_NUM_STATE 8
#define CASTRO_AMD_NGDNV 4
#define CASTRO_AMD_NUM_GROW 4

#define CASTRO_AMD_OK 0
#define CASTRO_AMD_ERR_ARG (-1)
#define CASTRO_AMD_ERR_UNSUPPORTED (-2)
#define CASTRO_AMD_ERR_NOMEM (-3)
#define CASTRO_AMD_ERR_HIP (-4)

/* FArrayBox descriptor: fab.dataPtr(), fab.loVect(), fab.hiVect(), fab.nComp() [AMReX] */
typedef struct castro_amd_fab {
    double *p;
    int lo[3];
    int hi[3];
    int ncomp;
} castro_amd_fab;

/* geom.data() + phys_bc (Castro::geom, Castro::phys_bc) */
typedef struct castro_amd_geom {
    double dx[3];        /* geom.CellSize() */
    double problo[3];    /* geom.ProbLo() */
    double probhi[3];    /* geom.ProbHi() */
    int domlo[3];        /* geom.Domain().loVect() */
    int domhi[3];        /* geom.Domain().hiVect() */
    int lo_bc[3];        /* phys_bc.lo(): 0 Interior 1 Inflow 2 Outflow 3 Symmetry 4 SlipWall 5 NoSlipWall */
    int hi_bc[3];        /* phys_bc.hi() */
    int coord;           /* geom.Coord(); only 0 (Cartesian) is supported */
} castro_amd_geom;

/* the castro:: runtime parameters the path reads (Source/driver/_cpp_parameters) */
typedef struct castro_amd_params {
    int ppm_type;                 /* 1 = PPM (default), 0 = PLM */
    int riemann_solver;           /* 0 CGF (default), 1 CG, 2 HLLC */
    int use_flattening;
    int hybrid_riemann;
    int first_order_hydro;
    int cg_maxiter;
    int cg_blend;                 /* 2 degrades to "keep last iterate" like the reference's GPU build */
    int transverse_use_eos;
    int transverse_reset_density;
    int transverse_reset_rhoe;
    int ppm_temp_fix;             /* 0 (default); 2 = EOS fix of the Riemann input states; 1 is a no-op in the CTU path */
    int plm_iorder;               /* 2 (default) or 1 */
    int plm_limiter;              /* 2 = 4th-order MC (default), 1 = 2nd-order MC */
    int use_pslope;               /* 1 (default): well-balanced pressure slope in PLM */
    double difmag;
    double small_dens, small_temp, small_pres, small_ener;
    double cg_tol;
    double dual_energy_eta1, dual_energy_eta2;
    double cfl, init_shrink, change_max;
    double eos_gamma;             /* gamma-law EOS (Microphysics EOS/gamma_law) */
    double small_x;
    double T_guess;
    double abar;                  /* mean molecular weight with eos_assume_neutral = 1 */
    double pslope_cutoff_density;
    int limit_fluxes_on_small_dens;   /* 0 (default); limit_hydro_fluxes_on_small_dens, advection_util.cpp:657-903 */
    int limit_fluxes_on_large_vel;    /* 0 (default); limit_hydro_fluxes_on_large_vel, :907-1075 (needs speed_limit > 0) */
    double speed_limit;               /* 0 (default: off); also enforce_speed_limit in clean_state, Castro.cpp:3049-3092 */
    int source_term_predictor;        /* 0 (default); 1: src_to_prim adds dt/2 x source_corrector to the momentum sources
                                       * (Castro_ctu.cpp:493-497); see castro_amd_ctx_set_source_corrector */
} castro_amd_params;

typedef struct castro_amd_ctx castro_amd_ctx;

/* Fill `p` with the reference defaults for the Sedov setup (see _cpp_parameters
 * and Exec/hydro_tests/Sedov/inputs.3d.sph*) and derive small_pres/small_ener
 * like Castro_setup.cpp:222-288. */
void castro_amd_default_params(castro_amd_params *p);
void castro_amd_finalize_params(castro_amd_params *p);

/* Context = scratch arena + device status word for one (device, stream). */
int castro_amd_ctx_create(castro_amd_ctx **ctx, int device);
void castro_amd_ctx_destroy(castro_amd_ctx *ctx);
/* Pre-allocate scratch for tiles up to nx*ny*nz valid cells (hipMalloc happens
 * here, never inside the calls below once reserved). */
int castro_amd_ctx_reserve(castro_amd_ctx *ctx, int nx, int ny, int nz);
/* Bytes of scratch currently held. */
long long castro_amd_ctx_scratch_bytes(const castro_amd_ctx *ctx);
/* Synchronises `stream`, returns and clears the latched device status bits:
 * bit0 = rho <= 0 or rho < small_dens met in ctoprim (advection_util.cpp:56-68). */
int castro_amd_ctx_status(castro_amd_ctx *ctx, void *stream);
/* Castro::source_corrector (a member MultiFab of the reference, Castro_advance.cpp:292-293, filled by
 * create_source_corrector, Castro.cpp:3780-3818): NSRC = 7 components on a box containing grow(bx, 3) of the tiles that
 * follow; the hydro calls on this context read it when params->source_term_predictor == 1.  NULL (or p == NULL)
 * clears it.  The caller owns the memory. */
int castro_amd_ctx_set_source_corrector(castro_amd_ctx *ctx, const castro_amd_fab *source_corrector);
/* Fill the scratch arena with NaNs (asynchronous on `stream`): lets a caller or a test prove that a call reads
 * nothing a previous call left behind. */
int castro_amd_ctx_poison_scratch(castro_amd_ctx *ctx, void *stream);

/* flags for castro_amd_ctu_hydro_fab */
#define CASTRO_AMD_UPDATE_ADD 0      /* S_new += dt*div(F)...   (reference semantics: S_new holds a copy of Sborder) */
#define CASTRO_AMD_UPDATE_FROM_SBORDER 1 /* S_new = Sborder + ... (elides MultiFab::Copy, Castro_advance_ctu.cpp:94) */
#define CASTRO_AMD_STAGE_A 4             /* only the part that reads no ghost zone of Sborder (ctoprim on bx, tracing on
                                          * grow(bx,-3)): may run while the halo exchange fills the ghost zones */
#define CASTRO_AMD_STAGE_B 8             /* the rest, after CASTRO_AMD_STAGE_A on the same context, tile and arguments */
/* The light split for the overlap of the halo exchange (round 6; not together with CASTRO_AMD_STAGE_A / _B):
 *   CASTRO_AMD_STAGE_VALID  only ctoprim -- with the sborder_clean_ntimes applications of clean_state -- on the zones of bx:
 *                           reads and writes NO ghost zone of Sborder, so it may run on one stream while the exchange fills
 *                           the ghost zones on another (after the exchange has packed: castro_amd_halo_plan_wait_packed);
 *   CASTRO_AMD_STAGE_REST   the rest, after CASTRO_AMD_STAGE_VALID on the same context, tile and arguments: ctoprim (+ the
 *                           cleans) on the ghost shell in ONE launch, then the whole un-split update;
 *   CASTRO_AMD_BC_FILL      the call fills the zones of grow(bx, 4) outside the problem domain in a non-periodic direction
 *                           itself (what castro_amd_bc_fill_fab does: FOEXTRAP / REFLECT_ODD per geom->lo_bc / hi_bc), from
 *                           in-domain zones it has cleaned already, and writes their primitive record in the same pass:
 *                           the caller passes Sborder with its same-level ghost zones exchanged and NO physical-boundary
 *                           fill.  clean_state is zone-local and even in the momenta, so "fill, then clean" (the
 *                           reference: Castro_advance.cpp:186) equals "clean, then fill"; every zone is cleaned
 *                           sborder_clean_ntimes times exactly.  Whole-box calls only.  CASTRO_AMD_ERR_UNSUPPORTED when a
 *                           mirrored ghost layer reaches past the in-domain zones of this FAB (a box thinner than its ghost
 *                           depth at a wall: fill with castro_amd_bc_fill_fab instead).
 * CASTRO_AMD_STAGE_REST with sborder_clean_ntimes > 0 needs CASTRO_AMD_BC_FILL (a boundary fill between the two stages
 * would copy zones that are clean already into zones the shell pass cleans again). */
#define CASTRO_AMD_STAGE_VALID 16
#define CASTRO_AMD_STAGE_REST 32
#define CASTRO_AMD_BC_FILL 64
#define CASTRO_AMD_FLUX_ASSIGN 2         /* flux_out[d] = 0 + dt*area*flux instead of +=: for callers that would zero
                                          * fluxes[d] just before this (one) hydro call of the step
                                          * (Castro_advance.cpp:391-394); elides that fill and the read of the RMW */

/*
 * The hot path: replaces the MFIter-loop body of Castro::construct_ctu_hydro_source
 * (Source/hydro/Castro_ctu_hydro.cpp:130-1480) for the tile bx = [bxlo, bxhi].
 *   vbxlo/vbxhi : valid box of the FAB the tile belongs to (mfi.validbox()); decides
 *                 mfi.nodaltilebox(d) (which shared faces this tile stores). Pass bx for whole-box calls.
 *   Sborder     : in, ncomp 8, box must contain grow(bx, 4)           (Castro::Sborder)
 *   src         : in, old_source (ncomp 7, box contains grow(bx,3)); p == NULL means identically zero
 *   S_new       : in/out on bx, ncomp 8                               (get_new_data(State_Type))
 *   flux_out[d] : in/out, += dt*area*flux on nodaltilebox(d), ncomp 8 (Castro::fluxes[d]); p NULL to skip
 *   mass_flux_out[d] : out, = scaled density flux, ncomp 1            (Castro::mass_fluxes[d]); p NULL to skip
 *   qe_out[d]   : out (optional, p NULL to skip), Godunov state u,v,w,p on the same faces, ncomp 4 (qe[d])
 * Returns CASTRO_AMD_ERR_ARG for boxes / component counts that do not fit, CASTRO_AMD_ERR_UNSUPPORTED for
 * non-Cartesian coordinates and for a tile or FAB whose component plane reaches 4 GiB (the
 * kernels address a plane with 32-bit byte offsets: tile boxes beyond ~800^3 zones).
 */
int castro_amd_ctu_hydro_fab(castro_amd_ctx *ctx,
                             const int bxlo[3], const int bxhi[3],
                             const int vbxlo[3], const int vbxhi[3],
                             const castro_amd_fab *Sborder,
                             const castro_amd_fab *src,
                             const castro_amd_fab *S_new,
                             const castro_amd_fab flux_out[3],
                             const castro_amd_fab mass_flux_out[3],
                             const castro_amd_fab qe_out[3],
                             const castro_amd_geom *geom,
                             const castro_amd_params *params,
                             double time, double dt, int flags, void *stream);

/*
 * castro_amd_ctu_hydro_fab followed, zone by zone and before S_new is written, by the sequence
 * do_advance_ctu runs on the updated state when no new-time source intervenes
 * (Source/driver/Castro_advance_ctu.cpp:168-225, 386-392):
 *   d_out[1] = min(d_out[1], density of the updated zone)         (S_new.min(URHO))
 *   clean_state applied `clean_ntimes` (>= 1) times               (Castro::clean_state)
 *   d_out[2] = min(d_out[2], dx/(c+|u|) of the zone cleaned ONCE) (Castro::estdt_cfl as the validity check of
 *                                                                  do_advance_ctu sees it, :386-392)
 *   d_out[0] = min(d_out[0], dx/(c+|u|) of the zone after the LAST clean_state)   (what estTimeStep of the next coarse
 *                                                                  step sees when post_timestep's clean_state rides along)
 * The result equals castro_amd_ctu_hydro_fab + castro_amd_clean_state_reduce_fab on bx, without the
 * second pass over S_new.  clean_ntimes == 0 is exactly castro_amd_ctu_hydro_fab; d_out may be NULL
 * (no reduction) and otherwise points to 3 device doubles initialised by the caller.
 */
int castro_amd_ctu_hydro_clean_fab(castro_amd_ctx *ctx,
                                   const int bxlo[3], const int bxhi[3],
                                   const int vbxlo[3], const int vbxhi[3],
                                   const castro_amd_fab *Sborder,
                                   const castro_amd_fab *src,
                                   const castro_amd_fab *S_new,
                                   const castro_amd_fab flux_out[3],
                                   const castro_amd_fab mass_flux_out[3],
                                   const castro_amd_fab qe_out[3],
                                   const castro_amd_geom *geom,
                                   const castro_amd_params *params,
                                   double time, double dt, int flags,
                                   int clean_ntimes, double *d_out, void *stream);

/*
 * The general form of the two calls above.  Fields beyond those of castro_amd_ctu_hydro_clean_fab:
 *   sborder_clean_ntimes  > 0: Castro::clean_state is applied that many times, IN PLACE, to every zone of
 *                         grow(bx, 4) of Sborder inside the pass that reads it (k_ctoprim) -- the clean_state(S_old) of
 *                         initialize_advance plus the clean_state(Sborder) after FillPatch
 *                         (Castro_advance.cpp:311, :186) without their own sweeps.  clean_state is zone-local, and
 *                         the ghost zones of a single level are copies (or mirror images) of valid zones, so
 *                         "FillPatch the uncleaned state, then clean everything" equals the reference's "clean, FillPatch,
 *                         clean".  Only for whole-box calls (bx == vbx, one tile per FAB: overlapping tiles would clean
 *                         shared ghost zones twice) without CASTRO_AMD_STAGE_A/B; Sborder is written (in the `contract`
 *                         build's default path, which reads neither afterwards, its temperature and species planes may
 *                         stay as they came).  With
 *                         CASTRO_AMD_STAGE_VALID the zones of bx are cleaned, with CASTRO_AMD_STAGE_REST the ghost shell
 *                         (pass the same count to both calls).
 *                         In the `contract` build (castro_amd_numerics()), on the default-solver path and together with
 *                         clean_ntimes > 0, the temperature and species components of Sborder are neither read nor
 *                         written back: nothing downstream depends on them (one species, gamma-law gas; the fused update
 *                         recomputes both for S_new) -- the other six components are cleaned in place as described.
 */
typedef struct castro_amd_hydro_opts {
    int flags;                  /* CASTRO_AMD_UPDATE_* | CASTRO_AMD_FLUX_ASSIGN | CASTRO_AMD_STAGE_* | CASTRO_AMD_BC_FILL */
    int clean_ntimes;           /* as in castro_amd_ctu_hydro_clean_fab */
    double *d_out;              /* as in castro_amd_ctu_hydro_clean_fab (device, THREE doubles) or NULL */
    int sborder_clean_ntimes;   /* see above; 0 = Sborder is read only */
    const double *d_dt;         /* not NULL: castro_amd_step_control's DEVICE vector `ctl` -- the kernels read the time step
                                 * from ctl[CASTRO_AMD_CTL_DTHYDRO] (the `dt` argument is ignored), and when
                                 * ctl[CASTRO_AMD_CTL_STATUS] != 0 (an earlier step of the batch was rejected) the call
                                 * leaves Sborder, S_new and the flux arrays untouched */
} castro_amd_hydro_opts;
int castro_amd_ctu_hydro_fab_ex(castro_amd_ctx *ctx,
                                const int bxlo[3], const int bxhi[3],
                                const int vbxlo[3], const int vbxhi[3],
                                const castro_amd_fab *Sborder,
                                const castro_amd_fab *src,
                                const castro_amd_fab *S_new,
                                const castro_amd_fab flux_out[3],
                                const castro_amd_fab mass_flux_out[3],
                                const castro_amd_fab qe_out[3],
                                const castro_amd_geom *geom,
                                const castro_amd_params *params,
                                double time, double dt, const castro_amd_hydro_opts *opts, void *stream);

/*
 * Host-free time stepping of a single level (no retries, no sources): one thread on the device does what the host does
 * between two hydro updates -- the tail of Castro::do_advance_ctu (Castro_advance_ctu.cpp:168-216, 386-392), the
 * time / step bookkeeping of Amr::coarseTimeStep and Castro::computeNewDt (Castro.cpp:1629-1819) for the next step:
 *   red (3 doubles, as written by castro_amd_ctu_hydro_clean_fab; reset to 1e200 on exit)
 *   ctl[CASTRO_AMD_CTL_DT]     in: the step just taken; out: the next step's dt
 *                              = min(cfl * red[0], change_max * dt) clipped to stop_time (fixed_dt > 0: fixed_dt)
 *   ctl[CASTRO_AMD_CTL_DTHYDRO] the dt the hydro kernels of that step use: dt, or with use_retry != 0 the single
 *                              subcycle of Castro::subcycle_advance_ctu, (time + dt) - time (Castro_advance_ctu.cpp:463-471),
 *                              which differs from dt in the last bit now and then; the validity check uses it too
 *   ctl[CASTRO_AMD_CTL_TIME]   += dt;   ctl[CASTRO_AMD_CTL_NSTEP] += 1
 *   ctl[CASTRO_AMD_CTL_STATUS] |= 1 if red[1] < small_dens (the step would be rejected),
 *                              |= 2 if change_max * cfl * red[2] < dt (timestep validity check); sticky: once set,
 *                              time, step count and dt stop changing, so that the host finds the first failure
 *   ctl[CASTRO_AMD_CTL_HIST + n % CASTRO_AMD_CTL_NHIST] = dt of step n (for hosts that want the sequence)
 * The hydro calls of the next step take their dt from ctl[CASTRO_AMD_CTL_DTHYDRO] (castro_amd_hydro_opts.d_dt = ctl).  The host
 * reads ctl when it wants to (one synchronisation per batch of steps instead of one per step).
 */
#define CASTRO_AMD_CTL_DT 0
#define CASTRO_AMD_CTL_TIME 1
#define CASTRO_AMD_CTL_NSTEP 2
#define CASTRO_AMD_CTL_STATUS 3
#define CASTRO_AMD_CTL_RHOMIN 4
#define CASTRO_AMD_CTL_EST 5
#define CASTRO_AMD_CTL_DTHYDRO 6
#define CASTRO_AMD_CTL_HIST 8
#define CASTRO_AMD_CTL_NHIST 56
#define CASTRO_AMD_CTL_SIZE 64
int castro_amd_step_control(castro_amd_ctx *ctx, double *d_red, double *d_ctl, const castro_amd_params *params,
                            double max_dt, double fixed_dt, double stop_time, int use_retry, void *stream);

/* Castro::clean_state on one FAB region (Source/driver/Castro.cpp:4238-4278):
 * enforce_min_density, normalize_species, reset_internal_energy, computeTemp,
 * applied `ntimes` times in a row to every zone of [lo,hi] (the reference runs it
 * up to three times back to back on the same zones between two hydro updates). */
int castro_amd_clean_state_fab(castro_amd_ctx *ctx, const castro_amd_fab *state,
                               const int lo[3], const int hi[3],
                               const castro_amd_params *params, int ntimes, void *stream);

/* The post-hydro sequence of Castro::do_advance_ctu fused into one pass over the zones of [lo,hi]:
 *   d_out[1] = min(d_out[1], min density of the state AS GIVEN)   (S_new.min(URHO), Castro_advance_ctu.cpp:168)
 *   clean_state applied `ntimes` times                            (Castro_advance_ctu.cpp:221-225)
 *   d_out[2] = min(d_out[2], min dx/(c+|u|) after the first application), d_out[0] = ... after the last
 *                                                                 (estTimeStep, Castro_advance_ctu.cpp:386)
 * d_out: device pointer to 3 doubles initialised by the caller (castro_amd_estdt_fab writes [0] and [1] only). */
int castro_amd_clean_state_reduce_fab(castro_amd_ctx *ctx, const castro_amd_fab *state,
                                      const int lo[3], const int hi[3], const castro_amd_geom *geom,
                                      const castro_amd_params *params, int ntimes, double *d_out, void *stream);

/* Gravity source terms for gravity.gravity_type = "ConstantGrav" (grav[] is the same in every zone,
 * Source/gravity/Gravity.cpp:860-866), castro.grav_source_type 1..4 (default 4):
 *   castro_amd_old_gravity_source_fab  Castro::construct_old_gravity_source, Source/gravity/Castro_gravity.cpp:234-362
 *   castro_amd_new_gravity_source_fab  Castro::construct_new_gravity_source, :384-596 (needs mass_fluxes[d] of the hydro call)
 *   castro_amd_saxpy_fab               Castro::apply_source_to_state (MultiFab::Saxpy), Source/sources/Castro_sources.cpp:10-19
 * `source` has NSRC = 7 components and is accumulated into (+=), as in the reference. */
int castro_amd_old_gravity_source_fab(castro_amd_ctx *ctx, const castro_amd_fab *state, const castro_amd_fab *source,
                                      const int lo[3], const int hi[3], const double grav[3], int grav_source_type,
                                      double dt, void *stream);
int castro_amd_new_gravity_source_fab(castro_amd_ctx *ctx, const castro_amd_fab *state_old, const castro_amd_fab *state_new,
                                      const castro_amd_fab *source, const castro_amd_fab mass_fluxes[3],
                                      const int lo[3], const int hi[3], const double grav[3], int grav_source_type,
                                      double dt, const castro_amd_geom *geom, void *stream);
/* dst = base + a * src[0:nsrc] (other components copied; base may be dst) followed by clean_state x clean_ntimes, one
 * pass: MultiFab::Copy(S_new, Sborder) + apply_source_to_state + clean_state of do_advance_ctu
 * (Castro_advance_ctu.cpp:94, 127-131, 262-268).  dst, base: ncomp 8. */
int castro_amd_apply_source_fab(castro_amd_ctx *ctx, const castro_amd_fab *dst, const castro_amd_fab *base, double a,
                                const castro_amd_fab *src, int nsrc, const int lo[3], const int hi[3],
                                const castro_amd_params *params, int clean_ntimes, void *stream);
int castro_amd_saxpy_fab(castro_amd_ctx *ctx, const castro_amd_fab *dst, double a, const castro_amd_fab *src, int ncomp,
                         const int lo[3], const int hi[3], void *stream);

/* Rotation source terms in the rotating frame (castro.do_rotation, state_in_rotating_frame = 1):
 *   castro_amd_old_rotation_source_fab  Castro::rsrc,     Source/rotation/rotation_sources.cpp:9-137
 *   castro_amd_new_rotation_source_fab  Castro::corrrsrc, :140-500 (implicit Coriolis update :186-237,318-355;
 *                                       rot_source_type 4 uses mass_fluxes[d] and the rotational potential,
 *                                       Source/rotation/Rotation.H:77-95)
 * omega = 2 pi / castro.rotational_period along castro.rot_axis (Rotation.H:10-22); center = problem::center. */
typedef struct castro_amd_rotation {
    double omega[3];
    double center[3];
    int include_centrifugal;        /* castro.rotation_include_centrifugal (default 1) */
    int include_coriolis;           /* castro.rotation_include_coriolis (1) */
    int rot_source_type;            /* castro.rot_source_type 1..4 (4) */
    int implicit_rotation_update;   /* castro.implicit_rotation_update (1) */
} castro_amd_rotation;
int castro_amd_old_rotation_source_fab(castro_amd_ctx *ctx, const castro_amd_fab *state, const castro_amd_fab *source,
                                       const int lo[3], const int hi[3], const castro_amd_rotation *rot,
                                       const castro_amd_geom *geom, double dt, void *stream);
int castro_amd_new_rotation_source_fab(castro_amd_ctx *ctx, const castro_amd_fab *state_old, const castro_amd_fab *state_new,
                                       const castro_amd_fab *source, const castro_amd_fab mass_fluxes[3],
                                       const int lo[3], const int hi[3], const castro_amd_rotation *rot,
                                       const castro_amd_geom *geom, double dt, void *stream);

/* The source stages of do_advance_ctu for EVERY box of a level in one call (the MFIter loops of do_old_sources /
 * do_new_sources, Source/sources/Castro_sources.cpp:230-349, around construct_ctu_hydro_source): a level of many small
 * boxes is bound by the host's launch rate, and these stages are three to four launches per box.  Per box, in this order:
 *   stage 0 (old time, Castro_advance_ctu.cpp:94, 127-131):  source = 0 (the whole FAB, ghost zones too);
 *            += old gravity source (grav != NULL); += old rotation source (rot != NULL);
 *            S_new = S_old + dt * source on [lo, hi], then clean_state x clean_ntimes      (castro_amd_apply_source_fab)
 *   stage 1 (new time, :262-268):  source = 0; += new gravity source; += new rotation source (both read S_old, S_new and
 *            mass_flux[d]);  S_new += dt * source on [lo, hi], then clean_state x clean_ntimes
 * with the arithmetic -- and the kernels -- of the single-box entry points above: the same bits.  stage 0: `source` is the
 * old-time Source_Type FAB with its ghost zones; stage 1: the new-time one (valid zones); mass_flux is read by stage 1 only.
 *   stage 1 | CASTRO_AMD_SOURCES_AFTER_REFLUX (the re-evaluation of the new-time sources after a reflux, Castro.cpp:2773-2868
 *             with update_sources_after_reflux; any other stage value, the bare 2 included, is CASTRO_AMD_ERR_ARG as before):
 *             S_new += -dt * source (the stored new-time source), clean_state x clean_ntimes, then stage 1 -- one launch, the
 *             bits of castro_amd_apply_source_fab(S_new, S_new, -dt, source) followed by stage 1.  `source` and mass_flux as
 *             in stage 1; dt is the dt of the advance that stored the source.  With a diffusion term (_ex, _opts):
 *             CASTRO_AMD_ERR_UNSUPPORTED -- its stencil reads the neighbours' S_new, which the one pass rewrites. */
typedef struct castro_amd_source_box {
    int lo[3], hi[3];
    castro_amd_fab S_old, S_new, source;
    castro_amd_fab mass_flux[3];
} castro_amd_source_box;
#define CASTRO_AMD_SOURCES_AFTER_REFLUX 16   /* OR-ed to stage 1 of castro_amd_sources_mf / _ex / _g / _opts */
int castro_amd_sources_mf(castro_amd_ctx *ctx, int stage, int nboxes, const castro_amd_source_box *boxes,
                          const double *grav /* [3] or NULL */, int grav_source_type, const castro_amd_rotation *rot /* or NULL */,
                          const castro_amd_geom *geom, const castro_amd_params *params, double dt, int clean_ntimes, void *stream);

/* Explicit thermal diffusion (castro.diffuse_temp = 1, Source/diffusion/): the term div(k grad T) added to (rho E) and (rho e)
 * at old and new time (Castro_diffusion.cpp:11-176) and the diffusion limit on the time step (timestep.cpp:259-345).
 * Constant conductivity only (conductivity.const_conductivity; the other conductivities of Microphysics are not restated).
 * The reference applies AMReX's MLABecLaplacian [3P, not in the reference tree]; what is evaluated here is this restatement,
 * NOT pinned against an AMReX build.  With T = state(UTEMP) as stored (it is not recomputed), per zone
 *   k_cc = diffuse_cond_scale_fac * (rho > cutoff ? const_conductivity * (rho < cutoff_hi ? (rho - cutoff) / (cutoff_hi - cutoff) : 1) : 0)
 *   bx(i) = 0.5 * (k_cc(i) + k_cc(i-1)),   fx = bx(i+1) * (T(i+1) - T(i)) - bx(i) * (T(i) - T(i-1)),   likewise fy, fz
 *   DiffTerm = fx / dx^2 + fy / dy^2 + fz / dz^2        (as dhx * fx + dhy * fy + dhz * fz, dhx = 1.0 / (dx * dx), left to right)
 * A face on a physical domain boundary (lo_bc / hi_bc != Interior) contributes a zero flux whatever its ghost zone holds (the
 * operator's Neumann condition, Diffusion.cpp:99-126); periodic and interior faces read the ghost zone, so `state` must hold
 * at least ONE filled ghost zone around [lo, hi].  Inflow on a low face, Symmetry on a high face (Dirichlet in the reference,
 * with an extrapolation of AMReX's that is not restated) and coord != 0 return CASTRO_AMD_ERR_UNSUPPORTED. */
typedef struct castro_amd_diffusion {
    double const_conductivity;          /* conductivity.const_conductivity */
    double diffuse_cutoff_density;      /* castro.diffuse_cutoff_density (default -1e200) */
    double diffuse_cutoff_density_hi;   /* castro.diffuse_cutoff_density_hi (default -1e200) */
    double diffuse_cond_scale_fac;      /* castro.diffuse_cond_scale_fac (default 1.0) */
} castro_amd_diffusion;
/* source(UEDEN) += mult * DiffTerm(state), source(UEINT) += mult * DiffTerm(state) on [lo, hi] (add_temp_diffusion_to_source);
 * diff_term (one component, or NULL): the bare DiffTerm as well (the reference's `diff_term` derive); source may be NULL then.
 * Only those two components of source and the one of diff_term are written, and only on [lo, hi].  An empty box (hi[d] < lo[d]
 * in some direction) launches nothing and returns CASTRO_AMD_OK.  CASTRO_AMD_ERR_ARG, with nothing written: state not of 8
 * components or not holding [lo, hi] grown by one; source of fewer than 6 components, diff_term not of exactly one, or either
 * not holding [lo, hi]; source and diff_term both NULL (_mf: any box without a source). */
int castro_amd_temp_diffusion_fab(castro_amd_ctx *ctx, const castro_amd_fab *state, const castro_amd_fab *source /* or NULL */,
                                  const castro_amd_fab *diff_term /* or NULL */, const int lo[3], const int hi[3],
                                  const castro_amd_diffusion *diff, const castro_amd_geom *geom, double mult, void *stream);
/* the same for every box of a level in ONE launch (a device table of the boxes is uploaded from host memory by the call) */
typedef struct castro_amd_diffusion_box {
    int lo[3], hi[3];
    castro_amd_fab state, source;
} castro_amd_diffusion_box;
int castro_amd_temp_diffusion_mf(castro_amd_ctx *ctx, int nboxes, const castro_amd_diffusion_box *boxes,
                                 const castro_amd_diffusion *diff, const castro_amd_geom *geom, double mult, void *stream);
/* Castro::estdt_temp_diffusion: d_out[0] = min(d_out[0], min over [lo, hi] of 0.5 * dx_d^2 / D), D = const_conductivity /
 * (rho c_v) with the RAW conductivity (no scale factor, no ramp) and c_v = k_B / ((gamma - 1) mu m_u); a zone with
 * rho <= diffuse_cutoff_density contributes max_dt / cfl.  d_out: ONE device double the caller initialised; the caller
 * multiplies the level minimum by cfl (Castro.cpp:1566-1590). */
int castro_amd_estdt_temp_diffusion_fab(castro_amd_ctx *ctx, const castro_amd_fab *state, const int lo[3], const int hi[3],
                                        const castro_amd_geom *geom, const castro_amd_params *params,
                                        const castro_amd_diffusion *diff, double max_dt, double *d_out, void *stream);

/* castro_amd_clean_state_reduce_fab / castro_amd_estdt_fab on the valid zones [lo, hi] of every box of a level, reduced
 * into ONE d_out (3 device doubles initialised by the caller): Castro_advance_ctu.cpp:168-225 and Castro::estTimeStep
 * (Castro.cpp:1507-1626) as one call per level. */
typedef struct castro_amd_state_box {
    int lo[3], hi[3];
    castro_amd_fab state;
} castro_amd_state_box;
int castro_amd_clean_state_reduce_mf(castro_amd_ctx *ctx, int nboxes, const castro_amd_state_box *boxes,
                                     const castro_amd_geom *geom, const castro_amd_params *params, int ntimes,
                                     double *d_out, void *stream);
int castro_amd_estdt_mf(castro_amd_ctx *ctx, int nboxes, const castro_amd_state_box *boxes,
                        const castro_amd_geom *geom, const castro_amd_params *params, double *d_out, void *stream);
int castro_amd_estdt_temp_diffusion_mf(castro_amd_ctx *ctx, int nboxes, const castro_amd_state_box *boxes,
                                       const castro_amd_geom *geom, const castro_amd_params *params,
                                       const castro_amd_diffusion *diff, double max_dt, double *d_out, void *stream);
/* castro_amd_sources_mf with the thermal-diffusion source in front of gravity and rotation, the reference's dispatch order
 * (diff_src, grav_src, rot_src: Castro_sources.cpp): stage 0 adds DiffTerm(S_old), stage 1 adds 0.5 * DiffTerm(S_new) and then
 * -0.5 * DiffTerm(S_old) to UEDEN and UEINT of the zeroed source before the other terms.  Two launches per stage: the stencil
 * goes first (the one-pass kernel writes S_new in place, and the new-time term reads the neighbours' S_new), the one-pass kernel
 * continues from the two components it left.  S_old needs one filled ghost zone around [lo, hi] at both stages (stage 1 reads
 * it for the old-time half of the corrector); S_new needs one at stage 1 only -- stage 0 writes its valid zones and reads none of
 * it.  A FAB without that zone is CASTRO_AMD_ERR_ARG, unsupported boundaries are CASTRO_AMD_ERR_UNSUPPORTED; every box of the
 * table is checked before the first launch, so a refused call has written nothing.  The source FAB need not be initialised: the
 * two energy components start from zero, the other components and the ghost zones of the FAB are zeroed.
 * diff == NULL: castro_amd_sources_mf, the same bits. */
int castro_amd_sources_mf_ex(castro_amd_ctx *ctx, int stage, int nboxes, const castro_amd_source_box *boxes,
                             const double *grav /* [3] or NULL */, int grav_source_type, const castro_amd_rotation *rot /* or NULL */,
                             const castro_amd_diffusion *diff /* or NULL */, const castro_amd_geom *geom,
                             const castro_amd_params *params, double dt, int clean_ntimes, void *stream);

/* The integrated quantities of Castro::sum_integrated_quantities (Source/driver/sum_integrated_quantities.cpp:60-230, built on
 * volWgtSum / locWgtSum, sum_utils.cpp:17-205) over the valid zones [lo, hi] of every box of a level, in ONE call:
 * d_out[CASTRO_AMD_DIAG_*] = sum over the zones of the quantity times vol = dx * dy * dz (coord 0 only).  With
 * loc_d = problo_d + (0.5 + index_d) * dx_d:
 *   MASS            rho                                      volWgtSum("density")
 *   XMOM .. ZMOM    (rho u)_d                                "xmom", "ymom", "zmom"
 *   ANGMOM_X .. _Z  ((loc - center) x (rho u))_d, the expression of the angular_momentum_* derives (CASTRO_AMD_DER_ANGMOM_*)
 *   RHO_E_INT       (rho e)                                  "rho_e"
 *   RHO_K           0.5 / rho * |rho u|^2, the expression of the kineng derive (CASTRO_AMD_DER_KINENG)
 *   RHO_E           (rho E)                                  "rho_E"
 *   COM_X .. _Z     (rho * loc_d)                            locWgtSum("density", d); the centre of mass is this over MASS
 *   SPECIES         (rho X)                                  volWgtSum("rho_" + species), NOT divided by M_solar
 * mask (or NULL: every zone counts): one byte per valid zone, shaped like [lo, hi], x fastest; a zero byte marks a zone
 * covered by a finer level.  The reference multiplies the derived field by build_fine_mask()'s 0 / 1 MultiFab
 * (sum_utils.cpp:29-33); here a covered zone is SKIPPED instead, so a NaN or Inf under a fine patch cannot poison the sum
 * (0 * NaN would) -- for finite data the two are the same number.  Ghost zones of the FABs are never read.
 * d_out is OVERWRITTEN (the caller initialises nothing; nboxes == 0 writes zeros).  The sum is taken in a fixed order --
 * per thread, across the lanes of a wave, across the waves of a workgroup, then over the workgroups' rows of partial sums
 * by a second launch -- and never through floating-point atomics: the same boxes give the same bits on every call and on
 * every stream.  The rows of partial sums live in the context (reserved at the first call, grown only by a call with more
 * workgroups than any before); apart from that the call neither allocates nor synchronises.
 * castro_amd_diag_workgroups: the number of workgroups (= rows of partial sums) the call launches for these boxes, or a
 * negative error; host arithmetic only. */
#define CASTRO_AMD_DIAG_N 14
#define CASTRO_AMD_DIAG_MASS 0
#define CASTRO_AMD_DIAG_XMOM 1
#define CASTRO_AMD_DIAG_YMOM 2
#define CASTRO_AMD_DIAG_ZMOM 3
#define CASTRO_AMD_DIAG_ANGMOM_X 4
#define CASTRO_AMD_DIAG_ANGMOM_Y 5
#define CASTRO_AMD_DIAG_ANGMOM_Z 6
#define CASTRO_AMD_DIAG_RHO_E_INT 7
#define CASTRO_AMD_DIAG_RHO_K 8
#define CASTRO_AMD_DIAG_RHO_E 9
#define CASTRO_AMD_DIAG_COM_X 10
#define CASTRO_AMD_DIAG_COM_Y 11
#define CASTRO_AMD_DIAG_COM_Z 12
#define CASTRO_AMD_DIAG_SPECIES 13
typedef struct castro_amd_diag_box {
    int lo[3], hi[3];
    castro_amd_fab state;
    const unsigned char *mask;
} castro_amd_diag_box;
int castro_amd_integrated_quantities_mf(castro_amd_ctx *ctx, int nboxes, const castro_amd_diag_box *boxes,
                                        const castro_amd_geom *geom, const double center[3],
                                        double *d_out /* CASTRO_AMD_DIAG_N device doubles, overwritten */, void *stream);
int castro_amd_diag_workgroups(int nboxes, const castro_amd_diag_box *boxes);

/* Monopole self-gravity, gravity.gravity_type = "MonopoleGrav" (Source/gravity/Gravity.cpp), 3-D Cartesian, one level, no
 * GR_GRAV.  n1d: bins of the radial arrays, drdxfac * (int(sqrt(nx^2 + ny^2 + nz^2)) + 2 * NUM_GROW) of the domain
 * (Castro.cpp:3887-3913, Gravity.cpp:315); drdxfac: gravity.drdxfac, the bins are dx[0] / drdxfac wide; center: problem::center;
 * max_radius_all_in_domain: min over d of probhi[d] - center[d] (Gravity.cpp:333-338); Gconst: the reference takes C::Gconst
 * from its Microphysics constants (cgs, 6.67428e-8 in that release) -- here it is the caller's. */
typedef struct castro_amd_monopole_params {
    int n1d, drdxfac;
    double center[3];
    double max_radius_all_in_domain;
    double Gconst;
} castro_amd_monopole_params;
/* Gravity::compute_radial_mass (Gravity.cpp:1409-1576) over the valid zones of every box: a zone under a zero mask byte (mask
 * as in castro_amd_diag_box), with rho == 0 (:1491) or whose centre lies beyond bin n1d - 1 (:1514) is skipped; every other
 * zone is split into drdxfac^3 sub-zones with the expressions of :1474-1541, and a sub-zone of bin index <= n1d - 1 adds
 * vol_frac * rho to the mass of its bin and counts one towards its volume; octant_factor = 8 when center sits on problo within
 * 1e-2 dx in all three directions (:1439-1447).  d_mass_vol: 2 * n1d device doubles, OVERWRITTEN: radial_mass, then radial_vol =
 * count * vol_frac (the reference adds vol_frac count times).  The bins are found without contraction in both builds, and the
 * masses are summed in an order fixed by the box table alone, never through floating-point atomics: the same boxes give
 * the same bits on every call and on every stream.  The result of a rank is ready for a sum over the ranks.  The rows of
 * partial sums and the device copy of the box table live in the context: a call with more workgroups or bins than any before,
 * or with a table the context has not seen, allocates and synchronises; any other call does neither and can be captured.
 * CASTRO_AMD_ERR_UNSUPPORTED: geom.coord != 0, or drdxfac above what a window of 64 bins per brick of 8 x 8 x 4 zones holds:
 * drdxfac * sqrt((8 dx)^2 + (8 dy)^2 + (4 dz)^2) / dx + 3 <= 64, i.e. drdxfac <= 5 for cubic zones. */
int castro_amd_radial_mass_mf(castro_amd_ctx *ctx, int nboxes, const castro_amd_diag_box *boxes, const castro_amd_geom *geom,
                              const castro_amd_monopole_params *params, double *d_mass_vol, void *stream);
/* The outward integration of Gravity::make_radial_gravity (Gravity.cpp:3170-3274) by one device thread: den = mass / vol where
 * vol > 0, the three branches around max_radius_all_in_domain, radial_grav[i] = -Gconst * mass_encl / rc^2.  d_mass_vol as
 * above (after the sum over the ranks), d_radial_grav: n1d device doubles.  No contraction in either build. */
int castro_amd_radial_gravity(castro_amd_ctx *ctx, const castro_amd_monopole_params *params, const castro_amd_geom *geom,
                              const double *d_mass_vol, double *d_radial_grav, void *stream);
/* Gravity::interpolate_monopole_grav (Gravity.cpp:1300-1406) onto the WHOLE box of grav_fab (3 components), ghost zones
 * included (:1322-1323): linear in bin 0 and in bin n1d - 1, quadratic with the min / max clamp between; a zone beyond bin
 * n1d - 1 is left as it is. */
int castro_amd_monopole_grav_fab(castro_amd_ctx *ctx, const double *d_radial_grav, const castro_amd_monopole_params *params,
                                 const castro_amd_geom *geom, const castro_amd_fab *grav_fab, void *stream);
/* castro_amd_old_gravity_source_fab / castro_amd_new_gravity_source_fab with the gravity of a zone read from 3-component FABs,
 * gold(i,j,k,n) and gnew(i,j,k,n) of Castro_gravity.cpp:234-362 and :384-596.  grav_source_type = 4 reads the six neighbours of
 * a zone (:564-574): grav_old and grav_new then hold one ghost zone around [lo, hi]. */
int castro_amd_old_gravity_source_gfab(castro_amd_ctx *ctx, const castro_amd_fab *state, const castro_amd_fab *source,
                                       const int lo[3], const int hi[3], const castro_amd_fab *grav_old, int grav_source_type,
                                       double dt, void *stream);
int castro_amd_new_gravity_source_gfab(castro_amd_ctx *ctx, const castro_amd_fab *state_old, const castro_amd_fab *state_new,
                                       const castro_amd_fab *source, const castro_amd_fab mass_fluxes[3],
                                       const int lo[3], const int hi[3], const castro_amd_fab *grav_old,
                                       const castro_amd_fab *grav_new, int grav_source_type,
                                       double dt, const castro_amd_geom *geom, void *stream);

/* Monopole gravity on the levels of an AMR hierarchy: Gravity::make_radial_gravity(level, time) (Gravity.cpp:2962-3168) bins
 * every level lev <= level at `time`, the zones under level lev + 1 masked for lev < level, and combines the arrays.
 *
 * castro_amd_radial_mass_mf_ex: castro_amd_radial_mass_mf over a state between two time levels, the branch
 * time > t_old && time < t_new of :2987-3000 (S = S_old * omalpha; S_new * alpha; S = S + S_new with alpha = (time - t_old) /
 * (t_new - t_old), omalpha = 1.0 - alpha): per box, rho = (state_old(URHO) * omalpha) + (state_new(URHO) * alpha), rounded in
 * that order with nothing fused, and the rho == 0 test of :1491 on that value.  Bricks, windows, summation orders, integer
 * volume counts, the drdxfac limit and its error code are castro_amd_radial_mass_mf's; a zone under a zero mask byte is
 * skipped (the reference multiplies the state by build_fine_mask and then skips on rho == 0: the same zones).  Which of old,
 * new or interpolated applies (the eps = (t_new - t_old) * 1e-6 tests of :2966-2986 and the abort of :3001) is the caller's
 * decision; for one time level it calls castro_amd_radial_mass_mf. */
typedef struct castro_amd_radial_box {
    int lo[3], hi[3];
    castro_amd_fab state_old, state_new;
    const unsigned char *mask;
    double omalpha, alpha;
} castro_amd_radial_box;
int castro_amd_radial_mass_mf_ex(castro_amd_ctx *ctx, int nboxes, const castro_amd_radial_box *boxes, const castro_amd_geom *geom,
                                 const castro_amd_monopole_params *params, double *d_mass_vol, void *stream);
/* The level combination of :3103-3168.  d_mass_vol[lev], lev = 0 .. level: the 2 * n1d[lev] device doubles of
 * castro_amd_radial_mass_mf(_ex) of level lev, already summed over the ranks.  d_out (2 * n1d[level] device doubles,
 * overwritten): radial_mass_summed, then radial_vol_summed of `level`: the level's own array, then for lev = level - 1 down
 * to 0, ratio = the product of the refinement ratios between lev and level (2 each), every bin i < n1d[level] / ratio of lev
 * adds (1. / double(ratio)) * array[lev][i] to the fine bins ratio * i .. ratio * i + ratio - 1.  One thread per fine bin
 * makes the reference's additions to that bin in the reference's order.  n1d differs per level (monopole_n1d of the level's
 * domain) and is no exact multiple of the coarser one: CASTRO_AMD_ERR_UNSUPPORTED when n1d[level] / ratio exceeds n1d[lev];
 * level < 16.  d_out feeds castro_amd_radial_gravity (geometry and n1d of `level`) and castro_amd_monopole_grav_fab. */
int castro_amd_radial_combine(castro_amd_ctx *ctx, int level, const double *const *d_mass_vol, const int *n1d, double *d_out,
                              void *stream);
/* The physical-boundary part of AmrLevel::FillPatch(Gravity_Type) (Gravity.cpp:894-900, 967-973): the zones of grav_fab (3
 * components) outside the domain in a non-periodic direction.  Components 0 / 1 / 2 carry the x / y / z velocity BC records
 * with inflow replaced (Castro_setup.cpp:614-622): first-order extrapolation at inflow and outflow faces, reflection at
 * symmetry faces and walls with the component normal to the face negated.  The image of a mirrored zone must lie inside
 * grav_fab (CASTRO_AMD_ERR_ARG otherwise).  The coarse-fine part of that FillPatch is CASTRO_AMD_OP_INTERP /
 * castro_amd_cc_interp_fab with 3 components. */
int castro_amd_grav_bc_fill_fab(castro_amd_ctx *ctx, const castro_amd_fab *grav_fab, const castro_amd_geom *geom, void *stream);

/* gravity.gravity_type = "PoissonGrav" on a single level: 3-D Cartesian, every face of the domain a Dirichlet face of the
 * potential (no periodic and no Symmetry face: CASTRO_AMD_ERR_UNSUPPORTED).  Everything is FP64 and runs on `stream` alone.
 *
 * The multipole boundary values (Gravity::fill_multipole_BCs, Gravity.cpp:1742-2216, with multipole_add, calcLegPolyL and
 * calcAssocLegPolyLM of Gravity_util.H and the factors of init_multipole_grav) with boundary_only = 1: every zone falls in the
 * last radial bin, so there is ONE set of moments.  Distances are divided by rmax = 0.5 * (the widest extent of the domain) *
 * sqrt(3), the volume of a zone by rmax^3; factArray(l, m) = 2 (l - m)! / (l + m)!; volumeFactor and the parity factors are 1.
 * lnum = gravity.max_multipole_order, 0 .. CASTRO_AMD_MAX_MULTIPOLE (above it: CASTRO_AMD_ERR_UNSUPPORTED; the reference stops
 * at lnum_max = 30). */
#define CASTRO_AMD_MAX_MULTIPOLE 16
typedef struct castro_amd_multipole {
    int lnum;
    double rmax;
    double center[3];             /* problem::center */
    double Gconst;
} castro_amd_multipole;
/* The moments of the density (component 0 of box.state) over the valid zones of `boxes`, masked zones skipped, into d_moments:
 * 3 (lnum + 1)^2 device doubles, overwritten, entry ((kind * (lnum + 1)) + l) * (lnum + 1) + m with kind 0 = qL0(l) (m = 0),
 * 1 = qLC(l, m), 2 = qLS(l, m), 1 <= m <= l; every other entry is zero.  Two stages in an order fixed by the box table, no
 * floating-point atomics: the same boxes give the same bits on every call, and on every stream as long as the calls of one
 * context are ordered by the host -- the context has ONE workspace of partial sums and one staged box table (as for
 * castro_amd_integrated_quantities_mf): a call that grows it synchronises its own stream only, and two calls in flight on two
 * streams would share it.
 * As in the reference (Gravity.cpp:1917), cosTheta = z / r has no guard: a zone whose centre coincides with `center` (an odd
 * extent with the centre in the middle of the domain) has r = 0 and gives NaN in every moment with l >= 1; lnum = 0 is not
 * affected (pow(0, 0) = 1 and cosTheta is not read).  Put the centre on a zone corner, or mask the zone. */
int castro_amd_multipole_moments_mf(castro_amd_ctx *ctx, int nboxes, const castro_amd_diag_box *boxes, const castro_amd_geom *geom,
                                    const castro_amd_multipole *mp, double *d_moments, void *stream);
/* The boundary potential (Gravity.cpp:2066-2216) of every zone of phi_fab (1 component) outside the domain -- faces, edges and
 * corners: phi = -G / rmax * sum(...  r^(-l-1) rmax^3) at the zone centre moved onto the domain face in every direction in which
 * the zone lies outside (i dx beyond the high face, (i + 1) dx below the low face); 0 where r < 1e-12.  Zones of the domain are
 * not written.  phi_fab must overlap the domain.  r^(-l-1) is pow(r, -l - 1) for l >= 1 and the division 1 / r for l = 0: with
 * lnum = 0 the values hold no library call and are the same bits wherever IEEE arithmetic is. */
int castro_amd_multipole_phi_bc_fab(castro_amd_ctx *ctx, const castro_amd_fab *phi_fab, const castro_amd_geom *geom,
                                    const castro_amd_multipole *mp, const double *d_moments, void *stream);
/* Geometric multigrid for lap(phi) = 4 pi G rho with the 7-point cell-centred Laplacian on the domain of `geom` (dx, dy, dz may
 * differ).  Level 0: the ghost zone of phi holds phi ON the domain face and the stencil's ghost is 2 phi_face - phi_inside
 * (AMReX's maxorder = 2 form); coarser levels are homogeneous.  Levels: coarsened by 2 while every extent is even and the
 * coarsened extent is at least 2.  A V-cycle: 2 red-black Gauss-Seidel sweeps, residual, restriction (the mean of the 8
 * children), the coarser levels, piecewise-constant prolongation, 2 sweeps; the coarsest level is 32 sweeps in one launch.
 * The plan owns the arrays of every level.  CASTRO_AMD_ERR_UNSUPPORTED when the coarsest level would hold more than
 * CASTRO_AMD_POISSON_MAX_BOTTOM zones (too few factors of 2 in the extents for this bottom solver), for a non-Cartesian
 * geometry and for a periodic or Symmetry face. */
#define CASTRO_AMD_POISSON_MAX_BOTTOM 4096
typedef struct castro_amd_poisson_plan castro_amd_poisson_plan;
int castro_amd_poisson_plan_create(castro_amd_ctx *ctx, const castro_amd_geom *geom, castro_amd_poisson_plan **plan);
void castro_amd_poisson_plan_destroy(castro_amd_ctx *ctx, castro_amd_poisson_plan *plan);
/* Solve from the phi the valid zones of phi_fab hold (1 component, the domain grown by one zone inside it; the ghost zones
 * outside the domain hold the boundary values), b = fourpiG * component rho_comp of rho_fab.  V-cycles until
 * ||r||_inf <= max(reltol * ||b||_inf, abstol * max(b)) (Gravity.cpp:3447-3558: setAlwaysUseBNorm(true), abs_eps = abs_tol *
 * max_rhs) or maxiter cycles; one norm is read back per cycle (the call synchronises `stream`).  *cycles: the cycles run (0 when
 * the start already meets the rule), *converged: 1 / 0, *final_norm: the last ||r||_inf.  h_history (host, maxiter + 3 doubles, or
 * NULL): ||b||_inf, max(b), the norm of the starting residual, then the norm after every cycle. */
int castro_amd_poisson_solve(castro_amd_ctx *ctx, castro_amd_poisson_plan *plan, const castro_amd_fab *phi_fab,
                             const castro_amd_fab *rho_fab, int rho_comp, double fourpiG, double reltol, double abstol, int maxiter,
                             int *cycles, int *converged, double *final_norm, double *h_history, void *stream);
/* One pass of the V-cycle on caller-owned FABs with the coefficients of level `level` of the plan (level 0: the domain; the box
 * of a coarser level is the coarsened domain).  phi-like FABs hold the level's box grown by one zone, the others the box.
 *   CASTRO_AMD_MG_SMOOTH    a = phi, b = rhs: one sweep of the zones with (i + j + k - lo) & 1 == colour
 *   CASTRO_AMD_MG_RESIDUAL  a = phi, b = rhs, c = residual (written)
 *   CASTRO_AMD_MG_RESTRICT  a = residual of `level`, b = rhs of level + 1 (written), c = phi of level + 1 (valid zones zeroed)
 *   CASTRO_AMD_MG_PROLONG   a = phi of level + 1, b = phi of `level` (added to)
 *   CASTRO_AMD_MG_NORM      a = any FAB on the box; d_out[0] = max |a|, d_out[1] = max a (device doubles) */
#define CASTRO_AMD_MG_SMOOTH 0
#define CASTRO_AMD_MG_RESIDUAL 1
#define CASTRO_AMD_MG_RESTRICT 2
#define CASTRO_AMD_MG_PROLONG 3
#define CASTRO_AMD_MG_NORM 4
int castro_amd_poisson_level_op(castro_amd_ctx *ctx, castro_amd_poisson_plan *plan, int op, int level, int colour,
                                const castro_amd_fab *a, const castro_amd_fab *b, const castro_amd_fab *c, double *d_out,
                                void *stream);
/* g = -grad(phi) (get_old / get_new_grav_vector, Gravity.cpp:874-878, over MLMG's getGradSolution) into the zones of the domain of
 * grav_fab (3 components): the mean of the two face gradients (phi_i - phi_{i-1}) / dx of a zone, negated; at a domain face the
 * linear ghost gives 2 (phi_1 - phi_face) / dx.  The zones outside the domain are left to castro_amd_grav_bc_fill_fab. */
int castro_amd_grad_phi_to_grav_fab(castro_amd_ctx *ctx, const castro_amd_fab *phi_fab, const castro_amd_fab *grav_fab,
                                    const castro_amd_geom *geom, void *stream);
/* Poisson gravity on a refined level that solves for itself (gravity.no_sync = 1, gravity.no_composite = 1, refinement ratio 2):
 * a patch [fine_lo, fine_hi] goes through the entry points above with a castro_amd_geom whose domlo / domhi are the patch (every
 * bc a Dirichlet one), and this call puts the Dirichlet data into the one-zone shell of the patch in phi_fine_fab (1 component,
 * the patch grown by one inside it).  The data come from the potential of the level below at the fine level's time,
 * c = (1 - a) * crse_old + a * crse_new (Gravity::GetCrsePhi; (1 - a) is formed first, then the two products, then the sum),
 * and are the value ON the fine face.  Beyond an x face, for the fine transverse indices (j, k): J = j >> 1, K = k >> 1, I_out
 * and I_in the coarse zones outside and inside the face,
 *   m(J, K) = 0.5 * (c(I_out, J, K) + c(I_in, J, K)),
 *   value = (m(J, K) + s_j * 0.125 * (m(J + 1, K) - m(J - 1, K))) + s_k * 0.125 * (m(J, K + 1) - m(J, K - 1)),
 * s = -1 for an even fine index and +1 for an odd one; the y and z faces alike, the lower transverse direction first.  The edge
 * and corner zones of the shell are set to 0 (no pass of the solver reads them); nothing else of phi_fine_fab is written.
 * Compiled without contraction in both numerics builds: the same bits.  CASTRO_AMD_ERR_ARG: a NULL or multi-component FAB, a
 * fine box that is not the refinement of a coarse box (an odd low or an even high corner), a non-finite a, the patch grown by
 * one not inside phi_fine_fab, or the coarsened patch grown by one not inside both coarse FABs. */
int castro_amd_poisson_cf_bc_fab(castro_amd_ctx *ctx, const castro_amd_fab *phi_fine_fab, const int fine_lo[3], const int fine_hi[3],
                                 const castro_amd_fab *crse_old_fab, const castro_amd_fab *crse_new_fab, double a, void *stream);
/* Poisson gravity on a refined level that is a union of SEVERAL boxes (tagged and clustered grids), all of them on this device:
 * the level is solved as ONE array over the bounding box BB of its disjoint boxes B_1 .. B_n, with a byte of coverage flags per
 * zone -- no exchange of phi between the boxes.  lo / hi: 3 ints per box, in the zones of the level; every box is the refinement
 * of a coarse box (even low, odd high corner) at non-negative indices.
 *
 * Multigrid level m lives on BB >> m; a zone of it is covered if it lies in some B_i >> m.  Level m + 1 exists while (a) lo and
 * hi + 1 of every box are divisible by 2^(m+1) -- the 8 children of a coarse zone are then all covered or all not --, (b) the
 * extents of BB >> m are even and their halves at least 2 (castro_amd_poisson_plan_create's rule), (c) fewer than 32 levels
 * exist.  Flags of a zone, made on the host at plan creation: bit 0 = covered; bit 1 + 2 d + side = the neighbour across the low
 * (side 0) / high (side 1) face of direction d is not covered (a zone beyond BB is not covered).
 * CASTRO_AMD_ERR_ARG: a box that is not such a refinement, two boxes that overlap.  CASTRO_AMD_ERR_UNSUPPORTED: the coarsest
 * level holds more than CASTRO_AMD_POISSON_MAX_BOTTOM zones of its bounding box.  Nothing is allocated or launched on a refusal.
 * The plan is freed by castro_amd_poisson_plan_destroy; the one-box entry points above refuse it (CASTRO_AMD_ERR_ARG), as the
 * entry points below refuse a plan of castro_amd_poisson_plan_create.
 *
 * Arrays.  phi_fab: 1 component, BB grown by one zone inside it.  faces_fab: 3 components, [BB.lo, BB.hi + 1] inside it;
 * component d at the zone (i, j, k) is the value of phi ON the low d-face of that zone (so the high x-face of (i, j, k) is the
 * entry (i + 1, j, k) of component 0).  It is read only where a flag bit is set: an uncovered zone at a concave corner of the
 * union is the neighbour of two covered zones across two faces with two values, so the values cannot live in phi's zones.
 *
 * The passes are those of castro_amd_poisson_solve with "beyond a domain face" replaced by "the flag of this face is set", f the
 * face value of level 0 and 0.0 on the coarser levels, and only covered zones written:
 *   smoother   dg = cdiag; low x: xm = 2.0 * f, dg = dg + cx; high x: xp = 2.0 * f, dg = dg + cx; then y, then z;
 *              p = (((cx * (xm + xp) + cy * (ym + yp)) + cz * (zm + zp)) - b) / dg; the colour of a zone is the parity of
 *              (ii + jj + kk) relative to the low corner of BB >> m; the bottom solve is 32 x (colour 0, colour 1) in one launch
 *   residual   across a flagged face the neighbour is 2.0 * f - p; lap = (cx * ((xm + xp) - 2.0 * p) + cy * ((ym + yp) - 2.0 * p))
 *              + cz * ((zm + zp) - 2.0 * p); r = b - lap
 *   restrict   on covered coarse zones: (((((((r000 + r100) + r010) + r110) + r001) + r101) + r011) + r111) * 0.125, phi_c = 0
 *   prolong    on covered fine zones: phi_f = phi_f + phi_c(ii / 2, jj / 2, kk / 2)
 *   norms      max |x| and max x over the covered zones
 *   rhs        b = fourpiG * component rho_comp of the state FAB of the box that holds the zone (rho_fabs[i] belongs to box i)
 * With this order a union that tiles a rectangular box gives, in the `exact` build, the bits of castro_amd_poisson_solve on that
 * box -- phi, norm history and cycle count -- unless the alignment of the tiles stops the coarsening before the extents do.
 * No floating-point atomics; everything on `stream`; one norm read back per V-cycle. */
int castro_amd_poisson_boxes_plan_create(castro_amd_ctx *ctx, const double dx[3], int nboxes, const int *lo, const int *hi,
                                         castro_amd_poisson_plan **plan);
/* The coarse-fine boundary values of the level: for every face of a covered zone of level 0 whose flag is set, the value of
 * castro_amd_poisson_cf_bc_fab for the face zone (the uncovered neighbour) -- the same formula, the same roundings, no
 * contraction in either build -- into the slot of that face in faces_fab.  A face between two boxes of the level and every other
 * slot is not written.  crse_old_fab / crse_new_fab (1 component each): the potentials of the level below; both must hold the
 * coarsened BB grown by one zone, of which the zones under the union grown by one are read.  CASTRO_AMD_ERR_ARG: a non-finite a,
 * a FAB that does not hold this. */
int castro_amd_poisson_boxes_cf_bc(castro_amd_ctx *ctx, castro_amd_poisson_plan *plan, const castro_amd_fab *faces_fab,
                                   const castro_amd_fab *crse_old_fab, const castro_amd_fab *crse_new_fab, double a, void *stream);
/* castro_amd_poisson_solve on the union: phi_fab holds the starting guess on the covered zones (the others are neither read nor
 * written), rho_fabs[i] the state of box i (nboxes: the plan's), its box inside it.  The outputs as castro_amd_poisson_solve. */
int castro_amd_poisson_boxes_solve(castro_amd_ctx *ctx, castro_amd_poisson_plan *plan, const castro_amd_fab *phi_fab,
                                   const castro_amd_fab *faces_fab, int nboxes, const castro_amd_fab *rho_fabs, int rho_comp,
                                   double fourpiG, double reltol, double abstol, int maxiter, int *cycles, int *converged,
                                   double *final_norm, double *h_history, void *stream);
/* g = -grad(phi) on the zones of box i into grav_fabs[i] (3 components, the box inside it): castro_amd_grad_phi_to_grav_fab's
 * arithmetic -- gl = (p - xm) / hx, gh = (xp - p) / hx, g_x = -(0.5 * (gl + gh)) --; a neighbour in a sibling box is an ordinary
 * neighbour, across a flagged face gl = (2.0 * (p - f)) / hx, gh = (2.0 * (f - p)) / hx.  Nothing outside the boxes is written. */
int castro_amd_grad_phi_to_grav_boxes(castro_amd_ctx *ctx, castro_amd_poisson_plan *plan, const castro_amd_fab *phi_fab,
                                      const castro_amd_fab *faces_fab, int nboxes, const castro_amd_fab *grav_fabs, void *stream);
/* castro_amd_poisson_level_op for a plan of a union: one masked pass on caller-owned FABs over BB >> level (phi-like FABs grown
 * by one zone).  faces_fab: the face values, level 0 only; NULL (required on a coarser level): every flagged face holds 0.0. */
int castro_amd_poisson_boxes_level_op(castro_amd_ctx *ctx, castro_amd_poisson_plan *plan, int op, int level, int colour,
                                      const castro_amd_fab *a, const castro_amd_fab *b, const castro_amd_fab *c,
                                      const castro_amd_fab *faces_fab, double *d_out, void *stream);
/* castro_amd_sources_mf with the gravity of every box read from its Gravity_Type FABs: grav_old[i] / grav_new[i] (3
 * components, one ghost zone around [lo, hi] of box i for grav_source_type = 4; grav_new is read by stage 1 only and may be
 * NULL for stage 0) take the place of the one vector -- the zone functions of castro_amd_old/new_gravity_source_gfab inside
 * the one-pass kernel.  Everything else as castro_amd_sources_mf. */
int castro_amd_sources_mf_g(castro_amd_ctx *ctx, int stage, int nboxes, const castro_amd_source_box *boxes,
                            const castro_amd_fab *grav_old, const castro_amd_fab *grav_new, int grav_source_type,
                            const castro_amd_rotation *rot /* or NULL */, const castro_amd_geom *geom,
                            const castro_amd_params *params, double dt, int clean_ntimes, void *stream);

/* The sponge (castro.do_sponge = 1, Source/sources/Castro_sponge.cpp): momentum is damped towards rho * target_velocity on the
 * time scale `timescale` wherever a sponge factor f in [lower_factor, upper_factor] is non-zero.  Per zone, from the NEW state:
 *   radial   (lower_radius >= 0 and upper_radius > lower_radius), r = |problo + (i + 1/2) dx - center|:
 *            f = lower_factor below lower_radius, upper_factor above upper_radius, between them
 *            lower_factor + 0.5 (upper_factor - lower_factor) (1 - cos(pi (r - lower_radius) / (upper_radius - lower_radius)))
 *   density  (both densities > 0; overrides the radial factor): lower_factor where rho > upper_density, upper_factor where
 *            rho < lower_density, the cosine ramp in (rho - upper_density) / (lower_density - upper_density) between them
 *   pressure (upper_pressure > 0 and lower_pressure >= 0; overrides both): the same in p = eos(rho, T, X) of the gamma law
 *   alpha = dt / timescale;  fac = -(1 - 1 / (1 + alpha f)) if implicit == 1, else -alpha f
 *   Sr[n] = (U[UMX + n] - rho * target_velocity[n]) * fac / dt;   SrE = sum_n U[UMX + n] * (1 / rho) * Sr[n]
 * and source(UMX + n) += Sr[n], source(UEDEN) += SrE; no other component is touched.  With lower == upper of a pair a zone
 * exactly on the threshold evaluates cos(pi * 0/0), as in the reference.  The sponge has no old-time source
 * (construct_old_sponge_source is empty).  The defaults of _cpp_parameters: radii, densities, pressures -1 (off),
 * lower_factor 0, upper_factor 1, target_velocity 0, implicit 1; the reference refuses timescale <= 0, and all three upper (or
 * all three lower) limits negative (Castro.cpp:475-488). */
typedef struct castro_amd_sponge {
    double lower_radius, upper_radius;          /* castro.sponge_lower_radius / _upper_radius */
    double lower_density, upper_density;        /* castro.sponge_lower_density / _upper_density */
    double lower_pressure, upper_pressure;      /* castro.sponge_lower_pressure / _upper_pressure */
    double lower_factor, upper_factor;          /* castro.sponge_lower_factor / _upper_factor */
    double target_velocity[3];                  /* castro.sponge_target_{x,y,z}_velocity */
    double timescale;                           /* castro.sponge_timescale */
    double center[3];                           /* problem::center */
    int implicit;                               /* castro.sponge_implicit */
} castro_amd_sponge;
/* Castro::construct_new_sponge_source / apply_sponge on [lo, hi] of one box: needs the new state and the Source_Type FAB only.
 * CASTRO_AMD_ERR_ARG unless geom->coord == 0, dt > 0 and sponge->timescale > 0. */
int castro_amd_new_sponge_source_fab(castro_amd_ctx *ctx, const castro_amd_fab *state_new, const castro_amd_fab *source,
                                     const int lo[3], const int hi[3], const castro_amd_sponge *sponge,
                                     const castro_amd_geom *geom, const castro_amd_params *params, double dt, void *stream);
/* The one-pass source stages with every source term of the three forms above behind one options struct, and the sponge:
 *   grav (a vector: castro_amd_sources_mf) or grav_old / grav_new (one FAB per box: castro_amd_sources_mf_g), not both;
 *   rot; diff (castro_amd_sources_mf_ex; not together with gravity FABs: CASTRO_AMD_ERR_UNSUPPORTED); sponge.
 * Every pointer may be NULL; with sponge == NULL the call IS the matching one of the three, the same bits.  With a sponge,
 * stage 1 adds its source after rotation (the dispatch order of Castro_sources.cpp:290-347) inside the one kernel, from the
 * S_new values the kernel loads for the apply -- the bits of castro_amd_new_sponge_source_fab called after the others; stage 0
 * accepts a sponge and adds nothing.  Argument checks as above. */
typedef struct castro_amd_source_opts {
    const double *grav;                         /* [3] or NULL */
    const castro_amd_fab *grav_old, *grav_new;  /* [nboxes] or NULL */
    int grav_source_type;
    const castro_amd_rotation *rot;
    const castro_amd_diffusion *diff;
    const castro_amd_sponge *sponge;
} castro_amd_source_opts;
int castro_amd_sources_mf_opts(castro_amd_ctx *ctx, int stage, int nboxes, const castro_amd_source_box *boxes,
                               const castro_amd_source_opts *opts, const castro_amd_geom *geom, const castro_amd_params *params,
                               double dt, int clean_ntimes, void *stream);

/* The central point mass of the gravity module (castro.use_point_mass = 1, castro.point_mass, castro.point_mass_fix_solution):
 * a mass M at problem::center whose field is added to the gravity vector of every gravity.gravity_type, ConstantGrav included.
 * M lives in ONE device double of the caller (d_point_mass): the kernels read it there and castro_amd_pointmass_apply_mf adds
 * to it, so an accreting run needs no host round trip between its steps.  3-D Cartesian: CASTRO_AMD_ERR_UNSUPPORTED unless
 * geom->coord == 0. */
typedef struct castro_amd_pointmass_params {
    double center[3];                           /* problem::center */
    double Gconst;                              /* C::Gconst */
} castro_amd_pointmass_params;
/* Gravity::add_pointmass_to_gravity (Source/gravity/Gravity.cpp:2903-2948, the phi part left out: there is no PhiGrav_Type
 * here) over the WHOLE box of grav_fab (3 components), ghost zones included -- the reference runs over the grown box.  Per zone
 *   x, y, z = problo + (i + 1/2) dx - center;  rsq = x*x + y*y + z*z;  radial_force = -Gconst * M / rsq;  rinv = 1 / sqrt(rsq)
 *   grav(n) += radial_force * (x_n * rinv)
 * in that order (`exact`: the bits of the expression; `contract`: with the build's FMA contraction).  The reference calls it at
 * the END of get_old_grav_vector / get_new_grav_vector (:902-907, :975-980): after interpolate_monopole_grav and after the
 * Gravity_Type FillPatch (castro_amd_grav_bc_fill_fab and the coarse-fine interpolation).  A zone whose centre coincides with
 * `center` divides by zero, as in the reference. */
int castro_amd_add_pointmass_fab(castro_amd_ctx *ctx, const castro_amd_fab *grav_fab, const castro_amd_pointmass_params *pm,
                                 const castro_amd_geom *geom, const double *d_point_mass, void *stream);
/* The same for grav_fabs[0 .. nfabs) -- the gravity FABs of the boxes of a level -- in one launch; the bits of nfabs
 * castro_amd_add_pointmass_fab calls.  The table is kept on the device by content: a call with a table the context has seen
 * neither allocates nor synchronises and can be captured into a graph. */
int castro_amd_add_pointmass_mf(castro_amd_ctx *ctx, int nfabs, const castro_amd_fab *grav_fabs,
                                const castro_amd_pointmass_params *pm, const castro_amd_geom *geom, const double *d_point_mass,
                                void *stream);
/* One box of Castro::pointmass_update: the valid zones [lo, hi] of the old and the new State_Type data (NUM_STATE components). */
typedef struct castro_amd_pointmass_box {
    int lo[3], hi[3];
    castro_amd_fab state_old, state_new;
} castro_amd_pointmass_box;
/* Castro::pointmass_update (Source/gravity/Castro_pointmass.cpp; called from Castro::advance, Castro_advance.cpp:102-107, on
 * the finest level when castro.point_mass_fix_solution = 1) in two stream-ordered halves with the sum over the ranks between
 * them.  The cube: icen = floor((center[d] - problo[d]) / dx[d] + 1e-8), the zones icen - 2 .. icen + 1 of every direction,
 * clipped to each box (:38-65).
 *   castro_amd_pointmass_delta_mf   *d_delta = sum over the cube zones of the boxes of dx*dy*dz * (state_new(URHO) -
 *                                   state_old(URHO)) (:67-86), OVERWRITTEN.  No floating-point atomics: one wave, the terms
 *                                   added in the order of the zone index inside the cube -- the same bits for any cut of the
 *                                   level into boxes, on every call and on every stream.  The boxes must be disjoint.
 *   (the caller sums *d_delta over the ranks: ParallelDescriptor::ReduceRealSum, :86)
 *   castro_amd_pointmass_apply_mf   if *d_delta > 0: *d_point_mass += *d_delta, and every cube zone of every box copies all
 *                                   NUM_STATE components from state_old to state_new (:88-153); otherwise nothing is written.
 * nboxes = 0 is accepted by both (a rank without a box of the level: delta 0, and the apply still moves the summed change into
 * its copy of the point mass).  Tables by content, as above. */
int castro_amd_pointmass_delta_mf(castro_amd_ctx *ctx, int nboxes, const castro_amd_pointmass_box *boxes,
                                  const castro_amd_pointmass_params *pm, const castro_amd_geom *geom, double *d_delta,
                                  void *stream);
int castro_amd_pointmass_apply_mf(castro_amd_ctx *ctx, int nboxes, const castro_amd_pointmass_box *boxes,
                                  const castro_amd_pointmass_params *pm, const castro_amd_geom *geom, const double *d_delta,
                                  double *d_point_mass, void *stream);

/* Tracer particles (castro.do_tracer_particles; Source/particles/CastroParticles.cpp).  The container is AMReX's
 * AmrTracerParticleContainer [3P, not in the reference tree]: AdvectWithUcc, Redistribute and the cloud-in-cell interpolation
 * are restated from the published algorithm and are NOT pinned against an AMReX build.  3-D Cartesian
 * (CASTRO_AMD_ERR_UNSUPPORTED unless geom->coord == 0).  The particles are the caller's device arrays, one entry per particle, in
 * an order these four calls never change (the migration calls below write new arrays); none of the four calls allocates
 * particle memory or synchronises.  The box tables are kept on the
 * device by content like those of the point mass.  n == 0 launches nothing and returns CASTRO_AMD_OK.
 *   id <= 0: an invalid particle -- never moved, sampled, counted or located again.
 *   level, grid: the level and the index of the box (in the level's table) where the particle lives, set by
 *                castro_amd_tracer_locate.
 *   r0..r2: the saved position between the two advection passes, the velocity of the corrector afterwards.
 *   cpu is not read (may be NULL).
 * d_flags: two device int32.  [0] += 1 for every particle and pass whose stencil had to be clamped to the array it reads (or
 * whose grid is no box of the table, or a box of the table without a FAB: that particle is skipped); [1] += 1 for every particle castro_amd_tracer_locate finds in no
 * box.  No input makes a call read or write outside a FAB; the caller reads the flags when it reads particle data. */
typedef struct castro_amd_tracers {
    long long n;
    double *x, *y, *z;
    double *r0, *r1, *r2;
    int *id, *cpu, *level, *grid;
} castro_amd_tracers;
/* One box of a level: a FAB with its ghost zones and the valid box inside it.  castro_amd_tracer_locate reads the valid box
 * only (fab.p may be NULL); castro_amd_tracer_count_mf takes fab.p as the address of int32 zones, one component.  In the tables
 * of advect, sample and count, fab.p == NULL marks a box another rank owns (the rest of `fab` is not read): a particle whose
 * grid names it is skipped -- advect and sample add 1 to flags[0] for it, count, which has no flags, drops it -- exactly as for
 * a grid outside the table.  After a migration no local particle names one. */
typedef struct castro_amd_tracer_box {
    castro_amd_fab fab;
    int vlo[3], vhi[3];
} castro_amd_tracer_box;
/* One pass (ipass = 0, 1) of AdvectWithUcc over the valid particles with level == `level`; boxes[b].fab is the state at
 * time + dt / 2 of box b (at least 4 components: URHO, UMX..UMZ), ghost zones filled.  The velocity of a stencil corner is
 * mom * (1.0 / rho) of that zone (CastroParticles.cpp:271-274), interpolated cell-centred cloud-in-cell in the index space of
 * the level:  l = (pos - problo) * (1 / dx) - 0.5, i = floor(l), f = l - i, s = {1 - f, f},
 *             val = sum over kk, jj, ii (in that nesting) of sx[ii] * sy[jj] * sz[kk] * data(i + ii, j + jj, k + kk).
 *   pass 0: r = pos; pos += 0.5 * dt * v          pass 1: pos = r + dt * v; r = v
 * Both numerics builds give the same bits (the file is compiled without contraction). */
int castro_amd_tracer_advect_mf(castro_amd_ctx *ctx, int level, int nboxes, const castro_amd_tracer_box *boxes,
                                const castro_amd_geom *geom, double dt, int ipass, const castro_amd_tracers *tracers,
                                int *d_flags, void *stream);
/* Redistribute(lev_min, lev_max, ngrow) over the valid particles with level >= lev_min.  boxes: the tables of levels
 * 0 .. nlev - 1 one after the other (nboxes_per_level[l] entries each), geoms[l] the geometry of level l (one problo / probhi and
 * boundary types for all).  Per particle: wrap into [problo, probhi) in every periodic direction (a result equal to probhi
 * becomes problo); outside the domain in any other direction: id = -id; else the first level from lev_max down to lev_min with
 * a valid box over the cell floor((pos - problo) * (1 / dx)) -- the lowest box index -- takes it; else, with ngrow > 0, the
 * lowest-index box of lev_min whose valid box grown by ngrow holds the cell; else flags[1] += 1 and level / grid stay. */
int castro_amd_tracer_locate(castro_amd_ctx *ctx, int lev_min, int lev_max, int ngrow, int nlev, const int *nboxes_per_level,
                             const castro_amd_tracer_box *boxes, const castro_amd_geom *geoms, const castro_amd_tracers *tracers,
                             int *d_flags, void *stream);
/* The cloud-in-cell interpolation above of components comps[0 .. ncomps) of boxes[b].fab at the positions of the valid
 * particles with level == `level`: d_out[c * n + particle].  Entries of other particles are not written. */
int castro_amd_tracer_sample_mf(castro_amd_ctx *ctx, int level, int nboxes, const castro_amd_tracer_box *boxes,
                                const castro_amd_geom *geom, int ncomps, const int *comps, const castro_amd_tracers *tracers,
                                double *d_out, int *d_flags, void *stream);
/* ParticleDerive: += 1 (32-bit integer atomics: the sums do not depend on the order) in the zone
 * floor((pos - problo) * (1 / dx)) of the int32 FAB count_boxes[grid] for every valid particle with level == `level`; a zone
 * outside that FAB is dropped.  The caller zeroes the FABs and converts them afterwards. */
int castro_amd_tracer_count_mf(castro_amd_ctx *ctx, int level, int nboxes, const castro_amd_tracer_box *count_boxes,
                               const castro_amd_geom *geom, const castro_amd_tracers *tracers, void *stream);
/* Migration of particles between ranks (the second half of Redistribute when the boxes are dealt over ranks): a stable
 * partition of a rank's particle arrays by destination rank, in three calls around the caller's transport.  A rank holds the
 * particles of the boxes it owns; `grid` stays the index in the level's global box list.  None of the calls synchronises or
 * allocates particle memory; the first keeps a scratch table in the context (grown behind `stream` when n grows).
 *   destination of a particle: owners[first box of its level + grid] if id > 0, 0 <= level < nlev and 0 <= grid <
 *   nboxes_per_level[level]; else myrank -- invalid particles and particles with no such box stay where they are.
 *   order: the particles that stay keep their order in tracers_out[0, nkeep); the leavers are wire records, contiguous per
 *   destination in ascending rank order, each group in its order in tracers_in.
 *   wire record: 64 bytes, eight 8-byte slots: the bits of x y z r0 r1 r2, then id | cpu << 32, then level | grid << 32 (the
 *   halves as unsigned 32-bit values; cpu travels as 0 when tracers_in->cpu is NULL).  d_wire is 16-byte aligned.
 * Errors: CASTRO_AMD_ERR_ARG for null pointers, myrank outside [0, nranks), an owner outside [0, nranks), n above 2^31 - 1 (the
 * counts are int32), at + nrecv > n; CASTRO_AMD_ERR_UNSUPPORTED for nranks > CASTRO_AMD_TRACER_MAX_RANKS (per-rank counters of
 * a workgroup live in LDS).  A refused call writes nothing.  Both numerics builds give the same bits (integer work and copies). */
#define CASTRO_AMD_TRACER_MAX_RANKS 256
/* d_dest[t] (n int32) and d_counts[r] (nranks int32): the destination of every particle and the number per destination
 * (d_counts[myrank]: the stayers).  owners: host ints, one per box, the levels one after the other.  n == 0 launches nothing
 * and zeroes d_counts. */
int castro_amd_tracer_migrate_count(castro_amd_ctx *ctx, int nlev, const int *nboxes_per_level, const int *owners, int nranks,
                                    int myrank, const castro_amd_tracers *tracers, int *d_dest, int *d_counts, void *stream);
/* The partition itself.  It relies on the scratch of the preceding castro_amd_tracer_migrate_count on the same context and
 * stream, with the same nranks, myrank, tracers_in and d_dest (CASTRO_AMD_ERR_ARG when n or nranks differ from that call's).
 * tracers_out: arrays of at least d_counts[myrank] entries (room for the arrivals may follow), none of them an array of
 * tracers_in; d_wire: nwire records,
 * nwire = the sum of the other d_counts (d_wire may be NULL when nwire == 0).  A particle whose place lies beyond
 * tracers_out->n or nwire -- sizes that do not belong to these counts -- is dropped, never written out of bounds. */
int castro_amd_tracer_migrate_pack(castro_amd_ctx *ctx, int nranks, int myrank, const castro_amd_tracers *tracers_in,
                                   const int *d_dest, const castro_amd_tracers *tracers_out, long long *d_wire, long long nwire,
                                   void *stream);
/* nrecv wire records into tracers_out[at, at + nrecv); nothing else is written.  nrecv == 0 launches nothing. */
int castro_amd_tracer_unpack(castro_amd_ctx *ctx, const long long *d_wire, long long nrecv, const castro_amd_tracers *tracers_out,
                             long long at, void *stream);

/* Checkpoints (castro_amd/checkpoint.py; for hosts without AMReX's own checkpoint writer): the valid zones of many ghosted FABs
 * into ONE contiguous buffer in the order of a FAB on disk -- x fastest, component slowest, entry after entry -- and back.
 *   castro_amd_pack_entry   fab: the (ghosted) FAB, ncomp >= 1; [vlo, vhi]: the region that is copied, inside the FAB's box;
 *                           offset: where the region's first double goes in the buffer (the region takes
 *                           ncomp x nx x ny x nz doubles; the caller keeps the regions of one call apart)
 *   castro_amd_fab_pack     copies every region to d_dst + offset.  d_minmax (or NULL): 2 x M doubles, M = the sum of ncomp over
 *                           the entries: the minimum of every (entry, component) in the order of the table, then the M maxima,
 *                           reduced from the values as they pass by two launches and no atomics.  A NaN in the region
 *                           propagates: the minimum and the maximum of its (entry, component) are then NaN.
 *   castro_amd_fab_unpack   the reverse copy: d_src + offset into the region; the zones of the FAB outside it are untouched.
 * Both return CASTRO_AMD_ERR_ARG for n < 0, a null pointer with n > 0, a region outside its FAB's box or empty, ncomp < 1 or a
 * negative offset; n == 0 returns 0 and launches nothing.
 * Like every table-driven call the two keep their device table and the rows of partial minima / maxima in the context: the calls
 * of ONE context must be ordered on ONE stream (a call that has to grow either buffer synchronises the stream it was given, not
 * others); use a context per stream for calls that may overlap. */
typedef struct {
    castro_amd_fab fab;
    int vlo[3], vhi[3];
    long long offset;
} castro_amd_pack_entry;
int castro_amd_fab_pack(castro_amd_ctx *ctx, int n, const castro_amd_pack_entry *entries, double *d_dst, double *d_minmax,
                        void *stream);
int castro_amd_fab_unpack(castro_amd_ctx *ctx, int n, const castro_amd_pack_entry *entries, const double *d_src, void *stream);

/* Two-level AMR building blocks, refinement ratio 2 (first slice).  The reference calls AMReX for
 * all of these [3P, not in the reference tree]; the arithmetic is restated from the published descriptions and is
 * NOT pinned against an AMReX build:
 *   castro_amd_cc_interp_fab          FillPatch coarse->fine with cell_cons_interp (Castro_setup.cpp:352-364): MC-limited
 *                                     slopes, one scaling factor per coarse zone keeping the children inside the range of
 *                                     the 27 neighbours; fills the fine zones [lo,hi]; crse must cover them grown by one
 *   castro_amd_lincomb_fab            dst = a x + b y  (time interpolation of the coarse data in FillPatch)
 *   castro_amd_avgdown_fab            amrex::average_down of Castro::avgDown (Castro.cpp:3096-3113) on coarse zones [lo,hi]
 *   castro_amd_fluxreg_crse_init_fab  FluxRegister::CrseInit of FluxRegCrseInit (Castro.cpp:2487-2512): reg = mult * flux
 *   castro_amd_fluxreg_fine_add_fab   FluxRegister::FineAdd of FluxRegFineAdd (:2516-2545): reg += mult * sum of 4 fine faces
 *   castro_amd_reflux_fab             FluxRegister::Reflux of Castro::reflux (:2549-2700): zones outside the faces [lo,hi]
 *                                     get -reg/vol (side 0, low face of the fine region) or +reg/vol (side 1)
 *   castro_amd_fluxreg_to_flux_fab    the coarse fluxes after the reflux (:2617-2644, castro.update_sources_after_reflux):
 *                                     flux += reg on the faces [lo,hi], ncomp components, and mass_flux = flux(URHO) there
 *                                     (mass_flux NULL or with p == NULL: the fluxes alone)
 *   castro_amd_error_tag_fab          amrex::AMRErrorTag of Castro::errorEst (Castro.cpp:3131-3164): kind 0 value_greater,
 *                                     1 value_less, 2 gradient, 3 relative_gradient on component `comp` of `field`
 *                                     (one ghost zone for the gradient kinds); tags (1 comp, 1.0 = tagged) are OR-ed
 *   castro_amd_fillpatch_shell_fab    the coarse-level part of a fine box's FillPatch in one launch: cc_interp into every
 *                                     zone of grow([vlo,vhi], ngrow) outside [vlo,vhi], followed by clean_state x
 *                                     clean_ntimes there (Castro_advance.cpp:186); ncomp 8
 * Register planes are ordinary FABs, one coarse face thick, in coarse face index space. */
/* Several independent FAB-to-FAB region operations in one launch (a level of many small boxes is launch-bound
 * otherwise: ~60 launches per box and advance).  The operations of one call must not write a zone that another one of
 * the same call reads or writes.  Kinds and their single-operation equivalents:
 *   CASTRO_AMD_OP_COPY               castro_amd_copy_fab              dst = src                (ncomp components)
 *   CASTRO_AMD_OP_LINCOMB            castro_amd_lincomb_fab           dst = a src + b src2
 *   CASTRO_AMD_OP_FLUXREG_CRSE_INIT  castro_amd_fluxreg_crse_init_fab dst = a src
 *   CASTRO_AMD_OP_FLUXREG_FINE_ADD   castro_amd_fluxreg_fine_add_fab  dst += a (sum of the 4 fine faces of src), dir
 *   CASTRO_AMD_OP_REFLUX             castro_amd_reflux_fab            dst zones outside the faces [lo,hi] -= / += src / a
 *   CASTRO_AMD_OP_AVGDOWN            castro_amd_avgdown_fab           dst = mean of the 8 fine zones of src (region in dst's index space)
 *   CASTRO_AMD_OP_FLUXREG_TO_FLUX    castro_amd_fluxreg_to_flux_fab   dst += src, and src2 = dst(URHO) where src2.p != NULL
 *                                                                      (side 0 / 1), a = zone volume */
#define CASTRO_AMD_OP_COPY 0
#define CASTRO_AMD_OP_LINCOMB 1
#define CASTRO_AMD_OP_FLUXREG_CRSE_INIT 2
#define CASTRO_AMD_OP_FLUXREG_FINE_ADD 3
#define CASTRO_AMD_OP_REFLUX 4
#define CASTRO_AMD_OP_CLEAN 5           /* Castro::clean_state x (int)a on the region of dst (ncomp 8); needs castro_amd_fab_ops_p.  Runs
                                         * the kernel of castro_amd_clean_state_fab (up to 32 regions per launch): the same bits as
                                         * that call in both numerics builds.  The CLEAN operations of a call are issued in front of
                                         * its other operations, whatever their place in the table; one with an empty region or
                                         * a == 0 does nothing */
#define CASTRO_AMD_OP_INTERP_CLEAN 6    /* dst (fine, ncomp 8) = cell_cons_interp of src (coarse data under it) on the region,
                                         * then clean_state x (int)a: one slab of a FillPatch ghost shell
                                         * (castro_amd_fillpatch_shell_fab does the six slabs of one box); castro_amd_fab_ops_p */
#define CASTRO_AMD_OP_AVGDOWN 7         /* dst (coarse) = mean of the 8 fine zones of src under each zone of the region (castro_amd_avgdown_fab):
                                         * Castro::avgDown of a whole level in one call */
#define CASTRO_AMD_OP_INTERP 8          /* dst (fine) = cell_cons_interp of src on the region, the first ncomp (<= 8) components, nothing else
                                         * (castro_amd_cc_interp_fab): the ghost shells of the Source_Type FillPatch of a level in one call */
#define CASTRO_AMD_OP_FLUXREG_TO_FLUX 9 /* dst (coarse flux) += src (register) on the faces of the region; src2: the mass-flux FAB that takes
                                         * component URHO of the sum, or p == NULL.  The registers of one orientation of a level in one call */
typedef struct castro_amd_fab_op {
    int kind;
    int dir;                     /* FLUXREG_FINE_ADD, REFLUX */
    int ncomp;
    int lo[3], hi[3];            /* region, in the index space of dst (REFLUX: the faces, in the index space of src) */
    int side;                    /* REFLUX only */
    double a, b;
    castro_amd_fab dst, src, src2;   /* src2: LINCOMB; FLUXREG_TO_FLUX (written, or p == NULL) */
} castro_amd_fab_op;
int castro_amd_fab_ops(castro_amd_ctx *ctx, int nops, const castro_amd_fab_op *ops, void *stream);
/* The same with the runtime parameters the CLEAN kinds need.  Any number of operations: up to sixteen travel as a kernel
 * argument, longer tables through a device buffer of the context, ONE launch either way -- the per-box sweeps of a level
 * of many small boxes (clean_state of every box, the ghost shells of every box) become one launch per level. */
int castro_amd_fab_ops_p(castro_amd_ctx *ctx, int nops, const castro_amd_fab_op *ops, const castro_amd_params *params,
                         void *stream);

/*
 * The MFIter loop itself (Source/hydro/Castro_ctu_hydro.cpp:130-1480): castro_amd_ctu_hydro_fab_ex for every box of a level
 * in one call.  Box i runs on ctxs[i % nctx] / streams[i % nctx] (each context has its own scratch; small boxes fill a
 * fraction of the chip, so several are kept in flight); the streams are forked from `stream` and joined to it with
 * events inside the call, so the caller sees one asynchronous operation on `stream`.  nctx == 1 with streams[0] == stream
 * is a plain loop.  opts applies to every box (d_out: one reduction vector for the level).
 */
typedef struct castro_amd_hydro_box {
    int bxlo[3], bxhi[3], vbxlo[3], vbxhi[3];
    castro_amd_fab Sborder, src, S_new;
    castro_amd_fab flux[3], mass_flux[3], qe[3];
} castro_amd_hydro_box;
int castro_amd_ctu_hydro_mf(castro_amd_ctx *const *ctxs, void *const *streams, int nctx,
                            const castro_amd_hydro_box *boxes, int nboxes,
                            const castro_amd_geom *geom, const castro_amd_params *params,
                            double time, double dt, const castro_amd_hydro_opts *opts, void *stream);

int castro_amd_fillpatch_shell_fab(castro_amd_ctx *ctx, const castro_amd_fab *crse, const castro_amd_fab *fine,
                                   const int vlo[3], const int vhi[3], int ngrow, const castro_amd_params *params,
                                   int clean_ntimes, void *stream);
int castro_amd_cc_interp_fab(castro_amd_ctx *ctx, const castro_amd_fab *crse, const castro_amd_fab *fine,
                             const int lo[3], const int hi[3], int ncomp, void *stream);
int castro_amd_error_tag_fab(castro_amd_ctx *ctx, const castro_amd_fab *field, int comp, const castro_amd_fab *tags,
                             const int lo[3], const int hi[3], int kind, double value, void *stream);
int castro_amd_lincomb_fab(castro_amd_ctx *ctx, const castro_amd_fab *dst, double a, const castro_amd_fab *x, double b,
                           const castro_amd_fab *y, int ncomp, const int lo[3], const int hi[3], void *stream);
int castro_amd_avgdown_fab(castro_amd_ctx *ctx, const castro_amd_fab *fine, const castro_amd_fab *crse,
                           const int lo[3], const int hi[3], int ncomp, void *stream);
int castro_amd_fluxreg_crse_init_fab(castro_amd_ctx *ctx, const castro_amd_fab *reg, const castro_amd_fab *crse_flux,
                                     const int lo[3], const int hi[3], int ncomp, double mult, void *stream);
int castro_amd_fluxreg_fine_add_fab(castro_amd_ctx *ctx, const castro_amd_fab *reg, const castro_amd_fab *fine_flux,
                                    const int lo[3], const int hi[3], int dir, int ncomp, double mult, void *stream);
int castro_amd_reflux_fab(castro_amd_ctx *ctx, const castro_amd_fab *state, const castro_amd_fab *reg,
                          const int lo[3], const int hi[3], int dir, int side, int ncomp, double vol, void *stream);
int castro_amd_fluxreg_to_flux_fab(castro_amd_ctx *ctx, const castro_amd_fab *flux, const castro_amd_fab *reg,
                                   const castro_amd_fab *mass_flux, const int lo[3], const int hi[3], int ncomp, void *stream);

/* Derived plotfile fields (Source/driver/Derive.cpp, registered in Castro_setup.cpp:756-960) for the
 * 3-D Cartesian gamma-law build.  Not provided: entropy (needs the Microphysics entropy formula),
 * StateErr, circvel, angular_momentum_{x,y,z}. */
enum {
    CASTRO_AMD_DER_PRESSURE = 0,   /* ca_derpres         Derive.cpp:24   */
    CASTRO_AMD_DER_KINENG,         /* ca_derkineng       :860 */
    CASTRO_AMD_DER_SOUNDSPEED,     /* ca_dersoundspeed   :180 */
    CASTRO_AMD_DER_GAMMA_1,        /* ca_dergamma1       :216 */
    CASTRO_AMD_DER_MACHNUMBER,     /* ca_dermachnumber   :251 */
    CASTRO_AMD_DER_MAGVORT,        /* ca_dermagvort      :929  (needs 1 ghost zone of state) */
    CASTRO_AMD_DER_DIVU,           /* ca_derdivu         :1021 (needs 1 ghost zone of state) */
    CASTRO_AMD_DER_EINT_E1,        /* eint_E, ca_dereint1 :57 */
    CASTRO_AMD_DER_EINT_E2,        /* eint_e, ca_dereint2 :79 */
    CASTRO_AMD_DER_LOGDEN,         /* ca_derlogden       :95 */
    CASTRO_AMD_DER_SPEC,           /* X(spec), ca_derspec :891 */
    CASTRO_AMD_DER_ABAR,           /* ca_derabar         :907 */
    CASTRO_AMD_DER_X_VELOCITY,     /* ca_dervel          :516 */
    CASTRO_AMD_DER_Y_VELOCITY,
    CASTRO_AMD_DER_Z_VELOCITY,
    CASTRO_AMD_DER_MAGVEL,         /* ca_dermagvel       :532 */
    CASTRO_AMD_DER_RADVEL,         /* ca_derradialvel    :572 (about `center`) */
    CASTRO_AMD_DER_MAGMOM,         /* ca_dermagmom       :692 */
    CASTRO_AMD_DER_STATEERR_0,     /* ca_derstate        :1087 (three components: density, Temp, X) */
    CASTRO_AMD_DER_STATEERR_1,
    CASTRO_AMD_DER_STATEERR_2,
    CASTRO_AMD_DER_CIRCVEL,        /* ca_dercircvel      :627 (about `center`, domain_is_plane_parallel = 0) */
    CASTRO_AMD_DER_ANGMOM_X,       /* ca_derangmomx/y/z  :711-870 (about `center`) */
    CASTRO_AMD_DER_ANGMOM_Y,
    CASTRO_AMD_DER_ANGMOM_Z,
    CASTRO_AMD_DER_COUNT
};
/* der(:,:,:,dcomp) = derived field `which` of `state` on [lo,hi]; `center` = problem::center (radvel only). */
int castro_amd_derive_fab(castro_amd_ctx *ctx, int which, const castro_amd_fab *state,
                          const castro_amd_fab *der, int dcomp, const int lo[3], const int hi[3],
                          const castro_amd_geom *geom, const castro_amd_params *params,
                          const double center[3], void *stream);

/* Castro::estdt_cfl (Source/driver/timestep.cpp:31-140) and S_new.min(URHO)
 * (Castro_advance_ctu.cpp:168) fused: d_out[0] = min over [lo,hi] of dx/(c+|u|)
 * (NOT yet multiplied by cfl), d_out[1] = min density.  d_out is a device
 * pointer to 2 doubles that the CALLER initialises (e.g. to +huge) so several
 * FABs can reduce into the same words. */
int castro_amd_estdt_fab(castro_amd_ctx *ctx, const castro_amd_fab *state,
                         const int lo[3], const int hi[3], const castro_amd_geom *geom,
                         const castro_amd_params *params, double *d_out, void *stream);

/* Physical-boundary ghost fill of a grown state FAB (the GpuBndryFuncFab /
 * ca_statefill part of AmrLevel::FillPatch: Source/problems/Castro_bc_fill_nd.cpp:11-125,
 * BC tables Source/driver/Castro_setup.cpp:40-53). Fills every zone of the FAB
 * outside the problem domain; x, then y, then z. */
int castro_amd_bc_fill_fab(castro_amd_ctx *ctx, const castro_amd_fab *state,
                           const castro_amd_geom *geom, void *stream);

/* The second half of ca_statefill (Source/problems/Castro_bc_fill_nd.cpp:41-105): the ambient fill
 * (Source/problems/ambient_fill.cpp:61-154), then the hydrostatic fill (Source/problems/hse_fill.cpp), in place, on a state
 * FAB whose zones outside the domain hold the generic fill already -- call it after castro_amd_bc_fill_fab, or after a
 * castro_amd_fill_boundary* that was given a geometry.  3-D Cartesian, gamma-law EOS.
 *   lo_type / hi_type      castro.{xl,yl,zl}_ext_bc_type / {xr,yr,zr}_ext_bc_type: -1 none, 1 HSE.  The hydrostatic fill runs on
 *                          a face only where its type is 1 AND its boundary is Inflow (the reference's EXT_DIR): every ghost
 *                          column of that face, ghost rows included, is integrated outward from the first zone inside the
 *                          domain with Newton's method on the density (at most 250 iterations, tolerance 1e-8 rho, every update
 *                          clamped to [0.9 rho, 1.1 rho]) under gravity.const_grav.
 *   hse_zero_vels, hse_interp_temp, hse_reflect_vels      the reference's parameters of those names
 *   fill_ambient_bc, ambient_fill_dir, ambient_outflow_vel: a zone beyond an Outflow face of direction ambient_fill_dir (-1:
 *                          any direction) takes ambient_state; with ambient_outflow_vel its normal momentum is the outgoing part
 *                          of the momentum of the first zone inside the domain, and UEDEN is made consistent.
 *   ambient_state          ambient::ambient_state (Castro_setup.cpp:339-350)
 * d_unconverged: NULL, or a device int to which every column that leaves a Newton loop unconverged adds 1 (the reference
 * aborts on the CPU and is silent on the GPU); the zone is written with the last iterate all the same.
 * Neither allocates nor synchronises.  Returns CASTRO_AMD_OK with nothing touched when state->ncomp != CASTRO_AMD_NUM_STATE
 * (a derive's fill, Castro_bc_fill_nd.cpp:47-49) or when the FAB holds no zone of the domain.  CASTRO_AMD_ERR_UNSUPPORTED:
 * geom->coord != 0; hi_type[2] == 1 on an Inflow +z face (hse_fill.cpp:988-991); two Inflow faces that meet at an edge
 * (Castro_bc_fill_nd.cpp:74-100).  CASTRO_AMD_ERR_ARG: hse_interp_temp or hse_reflect_vels on a face where the FAB holds
 * fewer zones of the domain than they read (two; as many as it has ghost layers). */
typedef struct castro_amd_ext_bc {
    int lo_type[3], hi_type[3];          /* -1 none, 1 HSE */
    int hse_zero_vels, hse_interp_temp, hse_reflect_vels;
    int fill_ambient_bc, ambient_fill_dir, ambient_outflow_vel;
    double const_grav;
    double ambient_state[8];
} castro_amd_ext_bc;
int castro_amd_ext_bc_fill_fab(castro_amd_ctx *ctx, const castro_amd_fab *state, const castro_amd_geom *geom,
                               const castro_amd_params *params, const castro_amd_ext_bc *ext, int *d_unconverged,
                               void *stream);

/* dst(lo:hi, 0:ncomp) = src(lo:hi, 0:ncomp) between two FABs (MultiFab::Copy /
 * the same-level copy part of FillPatch). */
int castro_amd_copy_fab(castro_amd_ctx *ctx, const castro_amd_fab *dst, const castro_amd_fab *src,
                        const int lo[3], const int hi[3], void *stream);

/* Pack / unpack a sub-box of a FAB to / from a contiguous buffer (same FAB
 * ordering restricted to the sub-box): the halo staging used by the RCCL
 * FillBoundary replacement. */
int castro_amd_pack_fab(castro_amd_ctx *ctx, const castro_amd_fab *fab, const int lo[3], const int hi[3],
                        double *buf, void *stream);
int castro_amd_unpack_fab(castro_amd_ctx *ctx, const castro_amd_fab *fab, const int lo[3], const int hi[3],
                          const double *buf, void *stream);

/* The same for all regions of one FillBoundary in ONE launch (a rank has up to 26 neighbours): region r is the box
 * lo[3r..3r+2] : hi[3r..3r+2] and lives at buf + offsets[r] (in doubles), r < nregions <= CASTRO_AMD_MAX_REGIONS. */
#define CASTRO_AMD_MAX_REGIONS 32
int castro_amd_pack_regions_fab(castro_amd_ctx *ctx, const castro_amd_fab *fab, int nregions, const int *lo, const int *hi,
                                const long long *offsets, double *buf, void *stream);
int castro_amd_unpack_regions_fab(castro_amd_ctx *ctx, const castro_amd_fab *fab, int nregions, const int *lo, const int *hi,
                                  const long long *offsets, const double *buf, void *stream);

/* Problem initial data on [lo,hi] of `state` (ncomp 8):
 * Exec/hydro_tests/Sedov/problem_initialize.H:8-113 + problem_initialize_state_data.H:8-148 */
int castro_amd_sedov_init_fab(castro_amd_ctx *ctx, const castro_amd_fab *state, const int lo[3], const int hi[3],
                              const castro_amd_geom *geom, const castro_amd_params *params,
                              double r_init, double p_ambient, double exp_energy, double dens_ambient,
                              int nsub, void *stream);
/* Exec/hydro_tests/Sod/problem_initialize*.H (use_Tinit = 0); idir is 1-based */
int castro_amd_sod_init_fab(castro_amd_ctx *ctx, const castro_amd_fab *state, const int lo[3], const int hi[3],
                            const castro_amd_geom *geom, const castro_amd_params *params,
                            double rho_l, double u_l, double p_l, double rho_r, double u_r, double p_r,
                            int idir, double frac, void *stream);

/*
 * FillBoundary on RCCL: the same-level ghost exchange of AmrLevel::FillPatch as Castro::expand_state uses it
 * (Source/driver/Castro.cpp:4201-4209) followed by the physical-boundary fill
 * (Source/problems/Castro_bc_fill_nd.cpp:11-125), for hosts without torch.distributed (castro_amd/csrc/halo_rccl.hip).
 * One rank per GPU; librccl is bound at run time (dlopen), so a single-GPU host never needs it.
 *
 *   castro_amd_comm        an RCCL communicator: created here from a 128-byte unique id that the host distributes with
 *                          whatever it has (MPI_Bcast, a file, torch.distributed), or adopted from the host's own ncclComm_t;
 *   castro_amd_halo_plan   the regions of ONE FAB shape (<= 26 neighbours), with the packed send / receive buffers: built
 *                          once per level and box, reused every step;
 *   castro_amd_fill_boundary   pack (1 launch) -> ncclGroupStart / ncclRecv.. / ncclSend.. / ncclGroupEnd -> unpack
 *                          (<= 2 launches) -> physical BC fill, all enqueued on `stream`: nothing synchronises, nothing allocates.
 *
 * A region sends the zones `sbox` of this rank's FAB to `peer` and receives the ghost zones `rbox` from the same peer
 * (equal shapes).  send_tag / recv_tag order the messages between a pair of ranks: the recv_tag of the region that
 * receives a message must equal the send_tag of the region that sent it (e.g. tag = 1 + ox + 3 (1 + oy) + 9 (1 + oz) of the
 * direction the message TRAVELS in).  peer == own rank (a periodic wrap onto this rank) is a local copy.
 *
 * A plan owns its two packed buffers (device memory outside any allocator of the host) until castro_amd_halo_plan_destroy,
 * which the owner calls once nothing of the plan is in flight; a plan is SINGLE-STREAM (two calls with one plan on two
 * streams would race on its buffers: one plan per stream and FAB shape).  castro_amd_fill_boundary selects the
 * communicator's device itself.
 */
typedef struct castro_amd_comm castro_amd_comm;
typedef struct castro_amd_halo_plan castro_amd_halo_plan;
#define CASTRO_AMD_UNIQUE_ID_BYTES 128
typedef struct castro_amd_halo_region {
    int peer;
    int sbox_lo[3], sbox_hi[3];
    int rbox_lo[3], rbox_hi[3];
    int send_tag, recv_tag;
} castro_amd_halo_region;
const char *castro_amd_comm_version(void);                       /* "RCCL x.y.z" of the library bound at run time */
int castro_amd_comm_unique_id(void *id);                         /* ncclGetUniqueId: id = CASTRO_AMD_UNIQUE_ID_BYTES host bytes */
int castro_amd_comm_create(castro_amd_comm **out, int nranks, int rank, const void *id, int device);   /* ncclCommInitRank (collective) */
int castro_amd_comm_adopt(castro_amd_comm **out, void *nccl_comm, int device);   /* wrap the host's ncclComm_t; not destroyed here */
int castro_amd_comm_rank(const castro_amd_comm *comm);
int castro_amd_comm_size(const castro_amd_comm *comm);
int castro_amd_comm_destroy(castro_amd_comm *comm);
int castro_amd_halo_plan_create(castro_amd_halo_plan **out, castro_amd_comm *comm, int nregions,
                                const castro_amd_halo_region *regions, int ncomp);
int castro_amd_halo_plan_destroy(castro_amd_halo_plan *plan);
long long castro_amd_halo_plan_bytes_sent(const castro_amd_halo_plan *plan);   /* bytes this rank sends to OTHER ranks per exchange */
/* geom == NULL: no physical-boundary fill (interior boxes of a level, or a caller that fills them itself) */
int castro_amd_fill_boundary(castro_amd_ctx *ctx, castro_amd_halo_plan *plan, const castro_amd_fab *state,
                             const castro_amd_geom *geom, void *stream);
/* castro_amd_fill_boundary for a caller that overlaps the exchange with work on another stream: the plan's "packed" event is
 * recorded on `stream` right behind the pack launch -- the LAST read of the valid zones of `state` by this call; everything after
 * it touches ghost zones only.  castro_amd_halo_plan_wait_packed makes `other_stream` wait for that event, after which work that
 * WRITES valid zones of `state` (CASTRO_AMD_STAGE_VALID with sborder_clean_ntimes > 0) may run on it beside the exchange.  Both
 * calls are capturable (the event becomes a dependency between the two streams of the graph).  flags: reserved, 0. */
int castro_amd_fill_boundary_ex(castro_amd_ctx *ctx, castro_amd_halo_plan *plan, const castro_amd_fab *state,
                                const castro_amd_geom *geom, int flags, void *stream);
int castro_amd_halo_plan_wait_packed(castro_amd_halo_plan *plan, void *other_stream);
/*
 * Several boxes per rank (round 6): ONE grouped exchange for all FABs of a level that this rank owns -- an AMR level, or two
 * boxes per GPU (Source/driver/Castro.cpp:4201-4209 over a BoxArray of any shape).  Sends and receives are separate lists:
 * with boxes of unequal size the zones a box sends to a neighbour and those it receives from it differ in shape.
 *   fab   index of the local FAB (0 .. nfabs-1) the zones [lo, hi] belong to
 *   peer  rank of the other end (own rank: a copy between two local boxes, or a periodic wrap; no RCCL call)
 *   tag   identifies the message between the two ranks: both ends must derive the same number for it, e.g.
 *         (source box * nboxes + destination box) * 27 + code of the periodic shift, box = index in the level's BoxArray
 * The k-th send to a peer in tag order is matched with the peer's k-th receive from this rank in tag order; two messages of
 * one pair of ranks with one tag are refused.  A local receive needs a local send of the same tag and size.
 * The group owns its two packed buffers; single-stream like a plan.  castro_amd_fill_boundary_group: states[f] is the FAB of
 * local box f; geom == NULL: no physical-boundary fill.
 */
typedef struct castro_amd_halo_group castro_amd_halo_group;
typedef struct castro_amd_halo_msg {
    int fab;
    int peer;
    int lo[3], hi[3];
    int tag;
} castro_amd_halo_msg;
int castro_amd_halo_group_create(castro_amd_halo_group **out, castro_amd_comm *comm, int nfabs,
                                 int nsends, const castro_amd_halo_msg *sends, int nrecvs, const castro_amd_halo_msg *recvs, int ncomp);
int castro_amd_halo_group_destroy(castro_amd_halo_group *group);
long long castro_amd_halo_group_bytes_sent(const castro_amd_halo_group *group);   /* bytes to OTHER ranks per exchange */
int castro_amd_fill_boundary_group(castro_amd_ctx *ctx, castro_amd_halo_group *group, const castro_amd_fab *states,
                                   const castro_amd_geom *geom, void *stream);
/* the overlap hooks of castro_amd_fill_boundary_ex / castro_amd_halo_plan_wait_packed for a group: the event is recorded behind
 * the LAST pack launch (the valid zones of every local FAB have been read by then).  flags: reserved, 0. */
int castro_amd_fill_boundary_group_ex(castro_amd_ctx *ctx, castro_amd_halo_group *group, const castro_amd_fab *states,
                                      const castro_amd_geom *geom, int flags, void *stream);
int castro_amd_halo_group_wait_packed(castro_amd_halo_group *group, void *other_stream);
/* ncclAllReduce(MIN) in place on n device doubles: the [dt estimate, min density, ...] reduction of a step */
int castro_amd_allreduce_min(castro_amd_comm *comm, double *d_buf, int n, void *stream);

/*
 * Grid generation of a regrid on the HOST (no device work, no context): the point clustering of Berger & Rigoutsos (1991) that
 * Amr::grid_places applies to the tags of Castro::errorEst (Source/driver/Castro.cpp:3131-3164) [3P: AMReX's ClusterList, restated
 * from the paper, not pinned against an AMReX build].  tags / mask: nz*ny*nx bytes, [z][y][x], non-zero = tagged / allowed
 * (mask NULL: everything allowed).  Every tagged, allowed cell ends up in exactly one box; a box lies inside the mask and is
 * filled to at least grid_eff with tags or is no longer than min_cells a side.  boxes: 6 ints per box (z0, y0, x0, z1, y1, x1),
 * inclusive.  Returns the number of boxes (only the first max_boxes are written: call again with a larger array if it is more)
 * or a negative error.  Same boxes as castro_amd/cluster.py::berger_rigoutsos (tests/test_cluster_cpu.py).
 */
int castro_amd_berger_rigoutsos(const unsigned char *tags, const unsigned char *mask, int nz, int ny, int nx,
                                double grid_eff, int min_cells, int *boxes, int max_boxes);

/* Library/version introspection */
const char *castro_amd_version(void);
/* CASTRO_AMD_ABI_VERSION the library was built with (see the macro above) */
int castro_amd_abi_version(void);
/* Numerics mode of this build of the library:
 *   "exact"    -ffp-contract=off, IEEE division / sqrt: bit-identical to the reference's CPU expression order ;
 *   "contract" FMA contraction, reciprocal-based division and rsq-based sqrt (<= 1 ulp each): agrees with `exact` to the
 *              north-star tolerance (rtol 1e-10 on every plotfile field, tests/test_gpu_parity.py) and is faster.
 * Both builds export the same ABI; castro_amd/_lib.py picks by CASTRO_AMD_NUMERICS. */
const char *castro_amd_numerics(void);
/* Name and average device time (ms) of the most recent launch of each hot-path
 * kernel when profiling is enabled with castro_amd_ctx_profile(ctx, 1): the
 * library brackets every kernel with hipEvents on `stream`. */
int castro_amd_ctx_profile(castro_amd_ctx *ctx, int enable);
int castro_amd_ctx_profile_count(castro_amd_ctx *ctx);
int castro_amd_ctx_profile_get(castro_amd_ctx *ctx, int idx, char *name, int name_len,
                               double *total_ms, long long *launches);
void castro_amd_ctx_profile_reset(castro_amd_ctx *ctx);

/*
 * Pointwise forms of the per-interface / per-zone functions of the path, for known-answer vectors recorded at the level
 * of the reference's own functions.  Flat lists of n points, device pointers, component-major: a[comp * n + point].
 * No context: nothing is allocated.
 *   castro_amd_cmpflx_points   body of Castro::cmpflx_plus_godunov for one interface (Source/hydro/riemann.cpp:62-203):
 *                              load_input_states (riemann.H:66-246), riemannus / riemanncg / HLLC (riemann_solvers.H),
 *                              compute_flux_q (:14-211), passive upwinding, HLL in shocked zones.
 *                              qm, qp: 7 comps (rho,u,v,w,p,rhoe,X); cl, cr: sound speed of the zones either side;
 *                              bnd_fac (NULL = 1) and is_shock (NULL = 0) per interface;
 *                              out: 11 comps (F_rho, F_mom normal/t/tt, F_E, F_eint, F_X, Godunov un, ut, utt, p)
 *   castro_amd_ppm_points      ppm_reconstruct (ppm.H:54-139) + ppm_int_profile (:157-252) of a five-point stencil
 *                              s (5 comps): out = (sm, sp, Ip[3], Im[3]) under the waves u-c, u, u+c
 *   castro_amd_flatten_points  the one-direction flattening coefficient of Castro::uflatten (flatten.cpp:12-166):
 *                              p7 = pressure at i-3..i+3, u5 = normal velocity at i-2..i+2
 *   castro_amd_trans_points    actual_trans_single (trans.cpp:66-437, ntrans = 1, tdir = transverse direction) or
 *                              actual_trans_final (:498-862, ntrans = 2): q 7 comps, flux records 8 comps
 *                              (rho, mx, my, mz, E, X fluxes, Godunov un, Godunov p) at the high (r) / low (l) face;
 *                              fe (NULL unless transverse_reset_rhoe = 1): the (rho e) fluxes at the faces 1r, 1l
 *                              (, 2r, 2l), rows of n
 */
int castro_amd_cmpflx_points(long long n, int idir, const double *qm, const double *qp, const double *cl, const double *cr,
                             const double *bnd_fac, const int *is_shock, const castro_amd_params *params, double *out,
                             void *stream);
int castro_amd_ppm_points(long long n, const double *s, const double *flatn, const double *u, const double *c, double dtdx,
                          double *out, void *stream);
int castro_amd_flatten_points(long long n, const double *p7, const double *u5, double *out, void *stream);
int castro_amd_trans_points(long long n, int ntrans, int tdir, const double *q, const double *f1r, const double *f1l,
                            const double *f2r, const double *f2l, const double *fe, double cdtdx1, double cdtdx2,
                            const castro_amd_params *params, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif

"""ctypes binding of castro_amd/libcastro_hydro_amd.so (the C ABI in include/castro_hydro_amd.h).

This module only loads the shared library and declares signatures.  There is NO
CPU fallback: if the library is missing, or no HIP device is present when a
context is created, it raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# Two builds of the same sources and the same ABI (castro_amd/csrc/Makefile):
#   exact     libcastro_hydro_amd.so            -ffp-contract=off, IEEE division / sqrt: bit-identical to the CPU restatement the tests check against
#   contract  libcastro_hydro_amd_contract.so   FMA contraction, reciprocal division, rsq-based sqrt: rtol 1e-10, faster
# CASTRO_AMD_NUMERICS picks the process default (exact); HipHydro(device, numerics=...) picks per context; both libraries can
# be loaded side by side.  CASTRO_AMD_LIB overrides the path for every mode (A/B builds).
NUMERICS_MODES = ("exact", "contract")
DEFAULT_NUMERICS = os.environ.get("CASTRO_AMD_NUMERICS", "exact")
_LIB_FILES = {"exact": "libcastro_hydro_amd.so", "contract": "libcastro_hydro_amd_contract.so"}


def lib_path(numerics=None):
    mode = numerics or DEFAULT_NUMERICS
    if mode not in NUMERICS_MODES:
        raise ValueError("CASTRO_AMD_NUMERICS / numerics must be one of %s, not %r" % (NUMERICS_MODES, mode))
    if os.environ.get("CASTRO_AMD_LIB"):             # A/B builds (tools/ab_variants.sh): one library whatever the mode asked for
        return os.environ["CASTRO_AMD_LIB"]
    return os.path.join(_HERE, _LIB_FILES[mode])


LIB_PATH = lib_path()

NUM_STATE, NGDNV, NUM_GROW = 8, 4, 4
URHO, UMX, UMY, UMZ, UEDEN, UEINT, UTEMP, UFS = range(8)

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_NOMEM, ERR_HIP = 0, -1, -2, -3, -4
UPDATE_ADD, UPDATE_FROM_SBORDER, FLUX_ASSIGN, STAGE_A, STAGE_B = 0, 1, 2, 4, 8
STAGE_VALID, STAGE_REST, BC_FILL = 16, 32, 64
# CASTRO_AMD_DER_* ids, in the order the reference registers the fields (Castro_setup.cpp:756-960)
DERIVE_IDS = {"pressure": 0, "kineng": 1, "soundspeed": 2, "Gamma_1": 3, "MachNumber": 4, "magvort": 5, "divu": 6,
              "eint_E": 7, "eint_e": 8, "logden": 9, "X(X)": 10, "abar": 11, "x_velocity": 12, "y_velocity": 13,
              "z_velocity": 14, "magvel": 15, "radvel": 16, "magmom": 17, "StateErr_0": 18, "StateErr_1": 19, "StateErr_2": 20,
              "circvel": 21, "angular_momentum_x": 22, "angular_momentum_y": 23, "angular_momentum_z": 24}

# every symbol include/castro_hydro_amd.h declares (checked by tests/test_capi_symbols.py)
EXPORTED_SYMBOLS = (
    "castro_amd_default_params", "castro_amd_finalize_params",
    "castro_amd_ctx_create", "castro_amd_ctx_destroy", "castro_amd_ctx_reserve",
    "castro_amd_ctx_scratch_bytes", "castro_amd_ctx_status", "castro_amd_ctx_poison_scratch", "castro_amd_ctx_set_source_corrector",
    "castro_amd_ctu_hydro_fab", "castro_amd_ctu_hydro_clean_fab", "castro_amd_ctu_hydro_fab_ex", "castro_amd_step_control", "castro_amd_ctu_hydro_mf", "castro_amd_fab_ops_p",
    "castro_amd_derive_fab",
    "castro_amd_error_tag_fab", "castro_amd_cc_interp_fab", "castro_amd_lincomb_fab", "castro_amd_avgdown_fab", "castro_amd_fluxreg_crse_init_fab",
    "castro_amd_fluxreg_fine_add_fab", "castro_amd_reflux_fab",
    "castro_amd_old_rotation_source_fab", "castro_amd_new_rotation_source_fab",
    "castro_amd_old_gravity_source_fab", "castro_amd_new_gravity_source_fab", "castro_amd_saxpy_fab", "castro_amd_clean_state_fab", "castro_amd_clean_state_reduce_fab",
    "castro_amd_estdt_fab", "castro_amd_sources_mf", "castro_amd_clean_state_reduce_mf", "castro_amd_estdt_mf",
    "castro_amd_bc_fill_fab", "castro_amd_copy_fab", "castro_amd_pack_fab", "castro_amd_unpack_fab",
    "castro_amd_pack_regions_fab", "castro_amd_unpack_regions_fab", "castro_amd_fillpatch_shell_fab", "castro_amd_apply_source_fab", "castro_amd_fab_ops",
    "castro_amd_sedov_init_fab", "castro_amd_sod_init_fab", "castro_amd_version", "castro_amd_abi_version", "castro_amd_numerics",
    "castro_amd_comm_version", "castro_amd_comm_unique_id", "castro_amd_comm_create", "castro_amd_comm_adopt", "castro_amd_comm_rank",
    "castro_amd_comm_size", "castro_amd_comm_destroy", "castro_amd_halo_plan_create", "castro_amd_halo_plan_destroy",
    "castro_amd_halo_plan_bytes_sent", "castro_amd_fill_boundary", "castro_amd_fill_boundary_ex", "castro_amd_halo_plan_wait_packed",
    "castro_amd_halo_group_create", "castro_amd_halo_group_destroy", "castro_amd_halo_group_bytes_sent", "castro_amd_fill_boundary_group",
    "castro_amd_fill_boundary_group_ex", "castro_amd_halo_group_wait_packed",
    "castro_amd_allreduce_min",
    "castro_amd_ctx_profile", "castro_amd_ctx_profile_count", "castro_amd_ctx_profile_get",
    "castro_amd_ctx_profile_reset",
    "castro_amd_berger_rigoutsos",
    "castro_amd_cmpflx_points", "castro_amd_ppm_points", "castro_amd_flatten_points", "castro_amd_trans_points",
    "castro_amd_temp_diffusion_fab", "castro_amd_temp_diffusion_mf", "castro_amd_estdt_temp_diffusion_fab",
    "castro_amd_estdt_temp_diffusion_mf", "castro_amd_sources_mf_ex",
    "castro_amd_integrated_quantities_mf", "castro_amd_diag_workgroups",
    "castro_amd_radial_mass_mf", "castro_amd_radial_gravity", "castro_amd_monopole_grav_fab",
    "castro_amd_old_gravity_source_gfab", "castro_amd_new_gravity_source_gfab",
    "castro_amd_radial_mass_mf_ex", "castro_amd_radial_combine", "castro_amd_grav_bc_fill_fab", "castro_amd_sources_mf_g",
    "castro_amd_new_sponge_source_fab", "castro_amd_sources_mf_opts",
    "castro_amd_add_pointmass_fab", "castro_amd_add_pointmass_mf", "castro_amd_pointmass_delta_mf", "castro_amd_pointmass_apply_mf",
    "castro_amd_ext_bc_fill_fab",
    "castro_amd_fluxreg_to_flux_fab",
    "castro_amd_tracer_advect_mf", "castro_amd_tracer_locate", "castro_amd_tracer_sample_mf", "castro_amd_tracer_count_mf",
    "castro_amd_tracer_migrate_count", "castro_amd_tracer_migrate_pack", "castro_amd_tracer_unpack",
    "castro_amd_fab_pack", "castro_amd_fab_unpack",
    "castro_amd_multipole_moments_mf", "castro_amd_multipole_phi_bc_fab", "castro_amd_poisson_plan_create",
    "castro_amd_poisson_plan_destroy", "castro_amd_poisson_solve", "castro_amd_poisson_level_op", "castro_amd_grad_phi_to_grav_fab",
    "castro_amd_poisson_cf_bc_fab",
    "castro_amd_poisson_boxes_plan_create", "castro_amd_poisson_boxes_cf_bc", "castro_amd_poisson_boxes_solve",
    "castro_amd_grad_phi_to_grav_boxes", "castro_amd_poisson_boxes_level_op",
)


class Fab(C.Structure):
    """castro_amd_fab: FArrayBox descriptor (pointer, lo, hi, ncomp)."""
    _fields_ = [("p", C.c_void_p), ("lo", C.c_int * 3), ("hi", C.c_int * 3), ("ncomp", C.c_int)]


# castro_amd_step_control's ctl vector (include/castro_hydro_amd.h)
CTL_DT, CTL_TIME, CTL_NSTEP, CTL_STATUS, CTL_RHOMIN, CTL_EST, CTL_DTHYDRO, CTL_HIST, CTL_NHIST, CTL_SIZE = 0, 1, 2, 3, 4, 5, 6, 8, 56, 64


class HaloRegion(C.Structure):
    """castro_amd_halo_region"""
    _fields_ = [("peer", C.c_int), ("sbox_lo", C.c_int * 3), ("sbox_hi", C.c_int * 3), ("rbox_lo", C.c_int * 3),
                ("rbox_hi", C.c_int * 3), ("send_tag", C.c_int), ("recv_tag", C.c_int)]


class HaloMsg(C.Structure):
    """castro_amd_halo_msg: one send or one receive of a many-box exchange (castro_amd_halo_group_create)"""
    _fields_ = [("fab", C.c_int), ("peer", C.c_int), ("lo", C.c_int * 3), ("hi", C.c_int * 3), ("tag", C.c_int)]


class HydroOpts(C.Structure):
    """castro_amd_hydro_opts"""
    _fields_ = [("flags", C.c_int), ("clean_ntimes", C.c_int), ("d_out", C.c_void_p), ("sborder_clean_ntimes", C.c_int),
                ("d_dt", C.c_void_p)]


class HydroBox(C.Structure):
    """castro_amd_hydro_box: one box of a castro_amd_ctu_hydro_mf call"""
    _fields_ = [("bxlo", C.c_int * 3), ("bxhi", C.c_int * 3), ("vbxlo", C.c_int * 3), ("vbxhi", C.c_int * 3),
                ("Sborder", Fab), ("src", Fab), ("S_new", Fab), ("flux", Fab * 3), ("mass_flux", Fab * 3), ("qe", Fab * 3)]


class SourceBox(C.Structure):
    """castro_amd_source_box: one box of a castro_amd_sources_mf call"""
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("S_old", Fab), ("S_new", Fab), ("source", Fab), ("mass_flux", Fab * 3)]


class StateBox(C.Structure):
    """castro_amd_state_box: one box of castro_amd_clean_state_reduce_mf / castro_amd_estdt_mf"""
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("state", Fab)]


class DiagBox(C.Structure):
    """castro_amd_diag_box: one box of a castro_amd_integrated_quantities_mf call"""
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("state", Fab), ("mask", C.c_void_p)]


# CASTRO_AMD_DIAG_*: the order of the sums castro_amd_integrated_quantities_mf writes (include/castro_hydro_amd.h)
DIAG_N = 14
(DIAG_MASS, DIAG_XMOM, DIAG_YMOM, DIAG_ZMOM, DIAG_ANGMOM_X, DIAG_ANGMOM_Y, DIAG_ANGMOM_Z, DIAG_RHO_E_INT, DIAG_RHO_K, DIAG_RHO_E,
 DIAG_COM_X, DIAG_COM_Y, DIAG_COM_Z, DIAG_SPECIES) = range(DIAG_N)
M_SOLAR = 1.9884e33        # C::M_solar of the reference's constants, cgs: species_diag.out is in solar masses


class MonopoleParams(C.Structure):
    """castro_amd_monopole_params"""
    _fields_ = [("n1d", C.c_int), ("drdxfac", C.c_int), ("center", C.c_double * 3), ("max_radius_all_in_domain", C.c_double),
                ("Gconst", C.c_double)]


class RadialBox(C.Structure):
    """castro_amd_radial_box: one box of a castro_amd_radial_mass_mf_ex call"""
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("state_old", Fab), ("state_new", Fab), ("mask", C.c_void_p),
                ("omalpha", C.c_double), ("alpha", C.c_double)]


MONOPOLE_MAX_LEVELS = 16       # castro_amd_radial_combine


# C::Gconst of the reference comes from its Microphysics constants; the cgs value of that release
GCONST = 6.67428e-8
# castro_amd_radial_mass_mf: a brick of 8 x 8 x 4 zones must fit a window of 64 bins (include/castro_hydro_amd.h)
MONOPOLE_BRICK, MONOPOLE_WINDOW = (8, 8, 4), 64


def monopole_n1d(n_cell, drdxfac):
    """bins of the radial arrays: drdxfac * (int(sqrt(nx^2 + ny^2 + nz^2)) + 2 * NUM_GROW) of the domain (Castro.cpp:3887-3913,
    Gravity.cpp:315)"""
    import math
    return int(drdxfac) * (int(math.sqrt(float(sum(int(n) * int(n) for n in n_cell)))) + 2 * NUM_GROW)


def monopole_max_drdxfac(dx):
    """the largest gravity.drdxfac the binning kernel takes for zones of size dx: drdxfac * (brick diagonal) / dx[0] + 3 <= 64"""
    import math
    diag = math.sqrt(sum((b * float(d)) ** 2 for b, d in zip(MONOPOLE_BRICK, dx)))
    return int((MONOPOLE_WINDOW - 3.0) * float(dx[0]) / diag)


def make_monopole(n_cell, geom, center, drdxfac=1, Gconst=GCONST, n1d=None):
    """castro_amd_monopole_params of a domain of n_cell zones: n1d (monopole_n1d unless given) and max_radius_all_in_domain =
    min over d of probhi[d] - center[d] (Gravity.cpp:333-338)"""
    if int(drdxfac) < 1:
        raise ValueError("gravity.drdxfac must be at least 1, not %r" % (drdxfac,))
    m = MonopoleParams()
    m.n1d = monopole_n1d(n_cell, drdxfac) if n1d is None else int(n1d)
    m.drdxfac = int(drdxfac)
    for d in range(3):
        m.center[d] = float(center[d])
    m.max_radius_all_in_domain = min(geom.probhi[d] - float(center[d]) for d in range(3))
    m.Gconst = float(Gconst)
    return m


class Multipole(C.Structure):
    """castro_amd_multipole"""
    _fields_ = [("lnum", C.c_int), ("rmax", C.c_double), ("center", C.c_double * 3), ("Gconst", C.c_double)]


MAX_MULTIPOLE = 16             # CASTRO_AMD_MAX_MULTIPOLE
POISSON_MAX_BOTTOM = 4096      # CASTRO_AMD_POISSON_MAX_BOTTOM
MG_SMOOTH, MG_RESIDUAL, MG_RESTRICT, MG_PROLONG, MG_NORM = range(5)       # CASTRO_AMD_MG_*


def multipole_rmax(geom):
    """multipole::rmax (Gravity.cpp:1735-1739): 0.5 * the widest extent of the domain * sqrt(3)"""
    import math
    width = geom.probhi[0] - geom.problo[0]
    width = max(width, geom.probhi[1] - geom.problo[1])
    width = max(width, geom.probhi[2] - geom.problo[2])
    return 0.5 * width * math.sqrt(float(3))


def make_multipole(geom, center, lnum=0, Gconst=GCONST):
    """castro_amd_multipole of a domain: gravity.max_multipole_order, rmax of the domain, problem::center, C::Gconst"""
    if int(lnum) < 0:
        raise ValueError("gravity.max_multipole_order must not be negative, not %r" % (lnum,))
    if int(lnum) > MAX_MULTIPOLE:
        raise ValueError("gravity.max_multipole_order = %d is above the %d this library is built for (CASTRO_AMD_MAX_MULTIPOLE)"
                         % (int(lnum), MAX_MULTIPOLE))
    m = Multipole()
    m.lnum, m.rmax, m.Gconst = int(lnum), multipole_rmax(geom), float(Gconst)
    for d in range(3):
        m.center[d] = float(center[d])
    return m


def poisson_level_extents(n_cell):
    """the extents of the multigrid levels of a domain of n_cell zones: coarsened by 2 while every extent is even and the
    coarsened extent is at least 2 (castro_amd_poisson_plan_create)"""
    n = tuple(int(x) for x in n_cell)
    out = [n]
    while all(x % 2 == 0 and x // 2 >= 2 for x in n) and len(out) < 32:
        n = tuple(x // 2 for x in n)
        out.append(n)
    return out


def poisson_boxes_levels(boxes):
    """[(lo, n) of the bounding box >> m] of the multigrid levels of a union of boxes (lo, hi), in the zones of the level
    (castro_amd_poisson_boxes_plan_create): coarsened while lo and hi + 1 of every box are divisible by 2^(m+1), every extent of
    the bounding box is even with a half of at least 2, and fewer than 32 levels exist"""
    lo = tuple(min(b[0][d] for b in boxes) for d in range(3))
    n = tuple(max(b[1][d] for b in boxes) - lo[d] + 1 for d in range(3))
    out = [(lo, n)]
    while (len(out) < 32 and all(x % 2 == 0 and x // 2 >= 2 for x in n)
           and all(b[0][d] % (1 << len(out)) == 0 and (b[1][d] + 1) % (1 << len(out)) == 0 for b in boxes for d in range(3))):
        lo, n = tuple(x >> 1 for x in lo), tuple(x // 2 for x in n)
        out.append((lo, n))
    return out


def poisson_boxes_alignment(boxes):
    """the largest power of 2 that divides lo and hi + 1 of every box"""
    k = 0
    while k < 30 and all(b[0][d] % (2 << k) == 0 and (b[1][d] + 1) % (2 << k) == 0 for b in boxes for d in range(3)):
        k += 1
    return 1 << k


class Rotation(C.Structure):
    """castro_amd_rotation"""
    _fields_ = [("omega", C.c_double * 3), ("center", C.c_double * 3), ("include_centrifugal", C.c_int),
                ("include_coriolis", C.c_int), ("rot_source_type", C.c_int), ("implicit_rotation_update", C.c_int)]


def make_rotation(rotational_period, rot_axis=3, center=(0.5, 0.5, 0.5), include_centrifugal=1, include_coriolis=1,
                  rot_source_type=4, implicit_rotation_update=1):
    """castro.rotational_period / castro.rot_axis -> omega (Source/rotation/Rotation.H:10-22)"""
    import math
    R = Rotation()
    for d in range(3):
        R.omega[d] = 0.0
        R.center[d] = center[d]
    if rotational_period > 0.0:
        R.omega[rot_axis - 1] = 2.0 * math.pi / rotational_period
    R.include_centrifugal, R.include_coriolis = include_centrifugal, include_coriolis
    R.rot_source_type, R.implicit_rotation_update = rot_source_type, implicit_rotation_update
    return R


class Sponge(C.Structure):
    """castro_amd_sponge"""
    _fields_ = [("lower_radius", C.c_double), ("upper_radius", C.c_double), ("lower_density", C.c_double),
                ("upper_density", C.c_double), ("lower_pressure", C.c_double), ("upper_pressure", C.c_double),
                ("lower_factor", C.c_double), ("upper_factor", C.c_double), ("target_velocity", C.c_double * 3),
                ("timescale", C.c_double), ("center", C.c_double * 3), ("implicit", C.c_int)]


def make_sponge(timescale, lower_radius=-1.0, upper_radius=-1.0, lower_density=-1.0, upper_density=-1.0, lower_pressure=-1.0,
                upper_pressure=-1.0, lower_factor=0.0, upper_factor=1.0, target_velocity=(0.0, 0.0, 0.0), center=None, implicit=1):
    """castro.do_sponge = 1 with the castro.sponge_* parameters and their defaults (Source/driver/_cpp_parameters:177-181,
    483-520) and the checks of Castro.cpp:475-488.  center: problem::center; None leaves it to the driver (its `center`
    attribute, else the middle of the domain) -- a direct caller of HipHydro.new_sponge_source gives it."""
    if not float(timescale) > 0.0:
        raise ValueError("If using the sponge, the sponge_timescale must be positive.")
    if max(float(upper_radius), float(upper_density), float(upper_pressure)) < 0.0:
        raise ValueError("If using the sponge, at least one of the upper radius, density, or pressure must be non-negative.")
    if max(float(lower_radius), float(lower_density), float(lower_pressure)) < 0.0:
        raise ValueError("If using the sponge, at least one of the lower radius, density, or pressure must be non-negative.")
    S = Sponge(float(lower_radius), float(upper_radius), float(lower_density), float(upper_density), float(lower_pressure),
               float(upper_pressure), float(lower_factor), float(upper_factor))
    for d in range(3):
        S.target_velocity[d] = float(target_velocity[d])
        S.center[d] = float(center[d]) if center is not None else float("nan")
    S.timescale, S.implicit = float(timescale), int(implicit)
    S.center_given = center is not None
    return S


class ExtBc(C.Structure):
    """castro_amd_ext_bc, and beside it the three runtime parameters the ambient state is built from (castro.ambient_density,
    ambient_temp, ambient_energy): they are no part of the C struct, which carries the finished ambient_state.  They default to
    the reference's -1e200 ("not set": the small_* quantities) on every instance, however it was made; copy() keeps them, a
    from_buffer_copy is a copy of the C struct alone and has the defaults again."""
    _fields_ = [("lo_type", C.c_int * 3), ("hi_type", C.c_int * 3), ("hse_zero_vels", C.c_int), ("hse_interp_temp", C.c_int),
                ("hse_reflect_vels", C.c_int), ("fill_ambient_bc", C.c_int), ("ambient_fill_dir", C.c_int),
                ("ambient_outflow_vel", C.c_int), ("const_grav", C.c_double), ("ambient_state", C.c_double * 8)]
    ambient_density = ambient_temp = ambient_energy = -1.e200

    def copy(self):
        E = ExtBc.from_buffer_copy(self)
        E.ambient_density, E.ambient_temp, E.ambient_energy = self.ambient_density, self.ambient_temp, self.ambient_energy
        return E


EXT_BC_TYPES = {"none": -1, "hse": 1, -1: -1, 1: 1}       # Source/problems/ext_bc_types.H: EXT_UNDEFINED, EXT_HSE
BC_INFLOW, BC_OUTFLOW = 1, 2


def ambient_state(params, ambient_density=-1.e200, ambient_temp=-1.e200, ambient_energy=-1.e200):
    """ambient::ambient_state (Castro_setup.cpp:339-350): the parameters where they were set, else the "small" quantities;
    UEDEN = UEINT, one species, momenta zero"""
    rho = max(float(ambient_density), params.small_dens)
    rhoe = rho * max(float(ambient_energy), params.small_ener)
    return (rho, 0.0, 0.0, 0.0, rhoe, rhoe, max(float(ambient_temp), params.small_temp), rho * (1.0 / 1))


def make_ext_bc(xl=-1, xr=-1, yl=-1, yr=-1, zl=-1, zr=-1, hse_zero_vels=0, hse_interp_temp=0, hse_reflect_vels=0,
                fill_ambient_bc=0, ambient_fill_dir=-1, ambient_outflow_vel=0, ambient_density=-1.e200, ambient_temp=-1.e200,
                ambient_energy=-1.e200):
    """castro.{xl,xr,yl,yr,zl,zr}_ext_bc_type ("hse" / 1, "none" / -1), castro.hse_*, castro.fill_ambient_bc and castro.ambient_*
    with the defaults of Source/driver/_cpp_parameters:193-253.  const_grav and ambient_state are completed by the driver
    (complete_ext_bc); a direct caller of HipHydro.ext_bc_fill sets them.  Raises ValueError for what
    castro_amd_ext_bc_fill_fab refuses whatever the geometry: HSE on +z, HSE faces that meet at an edge."""
    E = ExtBc()
    for d, (l, h) in enumerate(((xl, xr), (yl, yr), (zl, zr))):
        for v in (l, h):
            if isinstance(v, bool) or v not in EXT_BC_TYPES:
                raise ValueError("ext_bc_type %r: \"hse\" (1) or \"none\" (-1)" % (v,))
        E.lo_type[d], E.hi_type[d] = EXT_BC_TYPES[l], EXT_BC_TYPES[h]
    if E.hi_type[2] == 1:
        raise ValueError("HSE boundaries not implemented for +Z")
    if sum(E.lo_type[d] == 1 or E.hi_type[d] == 1 for d in range(3)) > 1:
        raise ValueError("external boundaries meeting at a corner not supported")
    if int(ambient_fill_dir) not in (-1, 0, 1, 2):
        raise ValueError("ambient_fill_dir: -1 (all), 0, 1 or 2")
    E.hse_zero_vels, E.hse_interp_temp, E.hse_reflect_vels = int(hse_zero_vels), int(hse_interp_temp), int(hse_reflect_vels)
    E.fill_ambient_bc, E.ambient_fill_dir, E.ambient_outflow_vel = int(fill_ambient_bc), int(ambient_fill_dir), int(ambient_outflow_vel)
    E.ambient_density, E.ambient_temp, E.ambient_energy = float(ambient_density), float(ambient_temp), float(ambient_energy)
    return E


def complete_ext_bc(ext, params, const_grav):
    """a copy of `ext` with gravity.const_grav and the ambient state of `params` (what a driver hands to the fill)"""
    E = ext.copy()
    E.const_grav = float(const_grav)
    for n, v in enumerate(ambient_state(params, ext.ambient_density, ext.ambient_temp, ext.ambient_energy)):
        E.ambient_state[n] = v
    return E


def ext_bc_hse_faces(ext, geom):
    """(direction, side) of the faces with a hydrostatic fill: of type HSE and Inflow (the reference's EXT_DIR)"""
    return [(d, s) for d in range(3) for s, (t, bc) in enumerate(((ext.lo_type[d], geom.lo_bc[d]), (ext.hi_type[d], geom.hi_bc[d])))
            if t == 1 and bc == BC_INFLOW]


def check_ext_bc(ext, geom):
    """ValueError for what castro_amd_ext_bc_fill_fab refuses with this geometry (its CASTRO_AMD_ERR_UNSUPPORTED and the
    domain-size part of CASTRO_AMD_ERR_ARG)"""
    if geom.coord != 0:
        raise ValueError("ext_bc: Cartesian geometry only")
    if sum(geom.lo_bc[d] == BC_INFLOW or geom.hi_bc[d] == BC_INFLOW for d in range(3)) > 1:
        raise ValueError("external boundaries meeting at a corner not supported")
    if geom.hi_bc[2] == BC_INFLOW and ext.hi_type[2] == 1:
        raise ValueError("HSE boundaries not implemented for +Z")
    for d, _ in ext_bc_hse_faces(ext, geom):
        if ext.hse_interp_temp == 1 and geom.domhi[d] - geom.domlo[d] + 1 < 2:
            raise ValueError("hse_interp_temp needs two zones of the domain in direction %d" % d)


class PointMassParams(C.Structure):
    """castro_amd_pointmass_params"""
    _fields_ = [("center", C.c_double * 3), ("Gconst", C.c_double)]


class PointMassBox(C.Structure):
    """castro_amd_pointmass_box: one box of castro_amd_pointmass_delta_mf / castro_amd_pointmass_apply_mf"""
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("state_old", Fab), ("state_new", Fab)]


def make_pointmass(center, Gconst=GCONST):
    """castro_amd_pointmass_params: problem::center and C::Gconst"""
    p = PointMassParams()
    for d in range(3):
        p.center[d] = float(center[d])
    p.Gconst = float(Gconst)
    return p


def pointmass_cube(center, geom):
    """(lo, hi) of the 4 x 4 x 4 zones Castro::pointmass_update sums over and restores (Castro_pointmass.cpp:38-65), before the
    clipping to a box: icen = floor((center - problo) / dx + 1e-8), icen - 2 .. icen + 1"""
    import math
    icen = [int(math.floor((float(center[d]) - geom.problo[d]) / geom.dx[d] + 1.e-8)) for d in range(3)]
    return tuple(i - 2 for i in icen), tuple(i + 1 for i in icen)


TRACER_MAX_RANKS = 256          # CASTRO_AMD_TRACER_MAX_RANKS


class Tracers(C.Structure):
    """castro_amd_tracers: the particle arrays on the device, one entry per particle"""
    _fields_ = [("n", C.c_longlong), ("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("r0", C.c_void_p),
                ("r1", C.c_void_p), ("r2", C.c_void_p), ("id", C.c_void_p), ("cpu", C.c_void_p), ("level", C.c_void_p),
                ("grid", C.c_void_p)]


def make_tracers(pos, r, ints):
    """castro_amd_tracers of device tensors: pos and r float64 (3, N) (rows x, y, z / r0, r1, r2), ints int32 (4, N) (rows id,
    cpu, level, grid); the tensors must outlive the struct"""
    import torch
    n = pos.shape[1]
    assert pos.dtype == torch.float64 and r.dtype == torch.float64 and ints.dtype == torch.int32
    assert pos.is_contiguous() and r.is_contiguous() and ints.is_contiguous()
    assert tuple(pos.shape) == (3, n) and tuple(r.shape) == (3, n) and tuple(ints.shape) == (4, n)
    t = Tracers()
    t.n = n
    t.x, t.y, t.z = (pos.data_ptr() + 8 * n * k for k in range(3))
    t.r0, t.r1, t.r2 = (r.data_ptr() + 8 * n * k for k in range(3))
    t.id, t.cpu, t.level, t.grid = (ints.data_ptr() + 4 * n * k for k in range(4))
    return t


class TracerBox(C.Structure):
    """castro_amd_tracer_box: a FAB of a box of a level and the valid box inside it"""
    _fields_ = [("fab", Fab), ("vlo", C.c_int * 3), ("vhi", C.c_int * 3)]


class PackEntry(C.Structure):
    """castro_amd_pack_entry: one FAB of a castro_amd_fab_pack / castro_amd_fab_unpack call"""
    _fields_ = [("fab", Fab), ("vlo", C.c_int * 3), ("vhi", C.c_int * 3), ("offset", C.c_longlong)]


class Diffusion(C.Structure):
    """castro_amd_diffusion"""
    _fields_ = [("const_conductivity", C.c_double), ("diffuse_cutoff_density", C.c_double),
                ("diffuse_cutoff_density_hi", C.c_double), ("diffuse_cond_scale_fac", C.c_double)]


def make_diffusion(const_conductivity, diffuse_cutoff_density=-1.e200, diffuse_cutoff_density_hi=-1.e200,
                   diffuse_cond_scale_fac=1.0):
    """castro.diffuse_temp = 1 with conductivity.const_conductivity and the castro.diffuse_* parameters
    (Source/driver/_cpp_parameters:401-416)"""
    return Diffusion(float(const_conductivity), float(diffuse_cutoff_density), float(diffuse_cutoff_density_hi),
                     float(diffuse_cond_scale_fac))


class DiffusionBox(C.Structure):
    """castro_amd_diffusion_box: one box of a castro_amd_temp_diffusion_mf call"""
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("state", Fab), ("source", Fab)]


class SourceOpts(C.Structure):
    """castro_amd_source_opts"""
    _fields_ = [("grav", C.POINTER(C.c_double)), ("grav_old", C.POINTER(Fab)), ("grav_new", C.POINTER(Fab)),
                ("grav_source_type", C.c_int), ("rot", C.POINTER(Rotation)), ("diff", C.POINTER(Diffusion)), ("sponge", C.POINTER(Sponge))]


# CODATA-2010 cgs constants of the gamma-law restatement (castro_amd/csrc/hydro_device.h)
K_B, M_U = 1.3806488e-16, 1.660538921e-24


def gamma_law_cv(params, xn=1.0):
    """c_v = e / T of the gamma-law gas, with the expressions of the kernels (eos_mu, eos_e_of_T)"""
    mu = 1.0 / (xn * (1.0 / params.abar))
    return K_B / ((params.eos_gamma - 1.0) * (mu * M_U))


class Geom(C.Structure):
    _fields_ = [("dx", C.c_double * 3), ("problo", C.c_double * 3), ("probhi", C.c_double * 3),
                ("domlo", C.c_int * 3), ("domhi", C.c_int * 3),
                ("lo_bc", C.c_int * 3), ("hi_bc", C.c_int * 3), ("coord", C.c_int)]


class Params(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "ppm_type", "riemann_solver", "use_flattening", "hybrid_riemann", "first_order_hydro",
        "cg_maxiter", "cg_blend", "transverse_use_eos", "transverse_reset_density",
        "transverse_reset_rhoe", "ppm_temp_fix", "plm_iorder", "plm_limiter", "use_pslope")] + \
        [(n, C.c_double) for n in (
            "difmag", "small_dens", "small_temp", "small_pres", "small_ener", "cg_tol",
            "dual_energy_eta1", "dual_energy_eta2", "cfl", "init_shrink", "change_max",
            "eos_gamma", "small_x", "T_guess", "abar", "pslope_cutoff_density")] + \
        [("limit_fluxes_on_small_dens", C.c_int), ("limit_fluxes_on_large_vel", C.c_int), ("speed_limit", C.c_double),
         ("source_term_predictor", C.c_int)]


class FabOp(C.Structure):
    """castro_amd_fab_op (include/castro_hydro_amd.h)"""
    _fields_ = [("kind", C.c_int), ("dir", C.c_int), ("ncomp", C.c_int), ("lo", C.c_int * 3), ("hi", C.c_int * 3),
                ("side", C.c_int), ("a", C.c_double), ("b", C.c_double), ("dst", Fab), ("src", Fab), ("src2", Fab)]


OP_COPY, OP_LINCOMB, OP_FLUXREG_CRSE_INIT, OP_FLUXREG_FINE_ADD, OP_REFLUX, OP_CLEAN, OP_INTERP_CLEAN, OP_AVGDOWN, OP_INTERP = 0, 1, 2, 3, 4, 5, 6, 7, 8
OP_FLUXREG_TO_FLUX = 9
SOURCES_AFTER_REFLUX = 16      # CASTRO_AMD_SOURCES_AFTER_REFLUX: OR-ed to stage 1 of the one-pass source stages

_libs = {}
ABI_VERSION = 5          # CASTRO_AMD_ABI_VERSION of include/castro_hydro_amd.h this binding was written against


def numerics_of(L):
    """"exact" / "contract" as the loaded library reports it (castro_amd_numerics)"""
    if not hasattr(L, "castro_amd_numerics"):
        return "exact"                                     # an A/B build of a revision before the second mode existed
    return L.castro_amd_numerics().decode()


def load(numerics=None):
    """Load the shared library of a numerics mode (raises if it has not been built)."""
    mode = numerics or DEFAULT_NUMERICS
    if mode in _libs:
        return _libs[mode]
    path = lib_path(mode)
    if not os.path.exists(path):
        raise ImportError(
            "castro_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C castro_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    L = C.CDLL(path)
    ab_build = bool(os.environ.get("CASTRO_AMD_LIB"))      # an A/B build, possibly of an older revision (tools/ab_variants.sh)
    if hasattr(L, "castro_amd_abi_version") or not ab_build:
        L.castro_amd_abi_version.restype = C.c_int
        if L.castro_amd_abi_version() != ABI_VERSION:
            raise ImportError("castro_amd: %s has ABI version %d, this binding expects %d: rebuild it"
                              % (path, L.castro_amd_abi_version(), ABI_VERSION))
        L.castro_amd_numerics.restype = C.c_char_p
        if not ab_build and numerics_of(L) != mode:
            raise ImportError("castro_amd: %s is a %r build, expected %r" % (path, numerics_of(L), mode))
    I3 = C.POINTER(C.c_int)
    PF = C.POINTER(Fab)
    L.castro_amd_version.restype = C.c_char_p
    L.castro_amd_default_params.argtypes = [C.POINTER(Params)]
    L.castro_amd_finalize_params.argtypes = [C.POINTER(Params)]
    L.castro_amd_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.castro_amd_ctx_destroy.argtypes = [C.c_void_p]
    L.castro_amd_ctx_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.castro_amd_ctx_scratch_bytes.restype = C.c_longlong
    L.castro_amd_ctx_scratch_bytes.argtypes = [C.c_void_p]
    L.castro_amd_ctx_status.argtypes = [C.c_void_p, C.c_void_p]
    L.castro_amd_ctx_poison_scratch.argtypes = [C.c_void_p, C.c_void_p]
    L.castro_amd_ctx_set_source_corrector.argtypes = [C.c_void_p, PF]
    L.castro_amd_ctu_hydro_fab.argtypes = [
        C.c_void_p, I3, I3, I3, I3, PF, PF, PF, PF, PF, PF, C.POINTER(Geom), C.POINTER(Params),
        C.c_double, C.c_double, C.c_int, C.c_void_p]
    L.castro_amd_ctu_hydro_clean_fab.argtypes = [
        C.c_void_p, I3, I3, I3, I3, PF, PF, PF, PF, PF, PF, C.POINTER(Geom), C.POINTER(Params),
        C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.castro_amd_ctu_hydro_fab_ex.argtypes = [
        C.c_void_p, I3, I3, I3, I3, PF, PF, PF, PF, PF, PF, C.POINTER(Geom), C.POINTER(Params),
        C.c_double, C.c_double, C.POINTER(HydroOpts), C.c_void_p]
    L.castro_amd_ctu_hydro_mf.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(HydroBox), C.c_int,
                                          C.POINTER(Geom), C.POINTER(Params), C.c_double, C.c_double, C.POINTER(HydroOpts),
                                          C.c_void_p]
    L.castro_amd_fab_ops_p.argtypes = [C.c_void_p, C.c_int, C.POINTER(FabOp), C.POINTER(Params), C.c_void_p]
    L.castro_amd_sources_mf.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(SourceBox), C.POINTER(C.c_double), C.c_int,
                                        C.POINTER(Rotation), C.POINTER(Geom), C.POINTER(Params), C.c_double, C.c_int, C.c_void_p]
    if hasattr(L, "castro_amd_temp_diffusion_fab"):         # absent from A/B builds of revisions before thermal diffusion
        PD = C.POINTER(Diffusion)
        L.castro_amd_temp_diffusion_fab.argtypes = [C.c_void_p, PF, PF, PF, I3, I3, PD, C.POINTER(Geom), C.c_double, C.c_void_p]
        L.castro_amd_temp_diffusion_mf.argtypes = [C.c_void_p, C.c_int, C.POINTER(DiffusionBox), PD, C.POINTER(Geom), C.c_double,
                                                   C.c_void_p]
        L.castro_amd_estdt_temp_diffusion_fab.argtypes = [C.c_void_p, PF, I3, I3, C.POINTER(Geom), C.POINTER(Params), PD,
                                                          C.c_double, C.c_void_p, C.c_void_p]
        L.castro_amd_estdt_temp_diffusion_mf.argtypes = [C.c_void_p, C.c_int, C.POINTER(StateBox), C.POINTER(Geom),
                                                         C.POINTER(Params), PD, C.c_double, C.c_void_p, C.c_void_p]
        L.castro_amd_sources_mf_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(SourceBox), C.POINTER(C.c_double), C.c_int,
                                               C.POINTER(Rotation), PD, C.POINTER(Geom), C.POINTER(Params), C.c_double, C.c_int,
                                               C.c_void_p]
    L.castro_amd_clean_state_reduce_mf.argtypes = [C.c_void_p, C.c_int, C.POINTER(StateBox), C.POINTER(Geom), C.POINTER(Params),
                                                   C.c_int, C.c_void_p, C.c_void_p]
    L.castro_amd_estdt_mf.argtypes = [C.c_void_p, C.c_int, C.POINTER(StateBox), C.POINTER(Geom), C.POINTER(Params), C.c_void_p, C.c_void_p]
    if hasattr(L, "castro_amd_integrated_quantities_mf"):   # absent from A/B builds of revisions before the integrated quantities
        L.castro_amd_integrated_quantities_mf.argtypes = [C.c_void_p, C.c_int, C.POINTER(DiagBox), C.POINTER(Geom),
                                                          C.POINTER(C.c_double * 3), C.c_void_p, C.c_void_p]
        L.castro_amd_diag_workgroups.argtypes = [C.c_int, C.POINTER(DiagBox)]
    if hasattr(L, "castro_amd_radial_mass_mf"):             # absent from A/B builds of revisions before monopole gravity
        PM = C.POINTER(MonopoleParams)
        L.castro_amd_radial_mass_mf.argtypes = [C.c_void_p, C.c_int, C.POINTER(DiagBox), C.POINTER(Geom), PM, C.c_void_p, C.c_void_p]
        L.castro_amd_radial_gravity.argtypes = [C.c_void_p, PM, C.POINTER(Geom), C.c_void_p, C.c_void_p, C.c_void_p]
        L.castro_amd_monopole_grav_fab.argtypes = [C.c_void_p, C.c_void_p, PM, C.POINTER(Geom), PF, C.c_void_p]
        L.castro_amd_old_gravity_source_gfab.argtypes = [C.c_void_p, PF, PF, I3, I3, PF, C.c_int, C.c_double, C.c_void_p]
        L.castro_amd_new_gravity_source_gfab.argtypes = [C.c_void_p, PF, PF, PF, PF, I3, I3, PF, PF, C.c_int, C.c_double,
                                                         C.POINTER(Geom), C.c_void_p]
    if hasattr(L, "castro_amd_radial_combine"):             # absent from A/B builds of revisions before monopole gravity on AMR levels
        PM = C.POINTER(MonopoleParams)
        L.castro_amd_radial_mass_mf_ex.argtypes = [C.c_void_p, C.c_int, C.POINTER(RadialBox), C.POINTER(Geom), PM, C.c_void_p, C.c_void_p]
        L.castro_amd_radial_combine.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        L.castro_amd_grav_bc_fill_fab.argtypes = [C.c_void_p, PF, C.POINTER(Geom), C.c_void_p]
        L.castro_amd_sources_mf_g.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(SourceBox), PF, PF, C.c_int,
                                              C.POINTER(Rotation), C.POINTER(Geom), C.POINTER(Params), C.c_double, C.c_int, C.c_void_p]
    if hasattr(L, "castro_amd_sources_mf_opts"):            # absent from A/B builds of revisions before the sponge
        L.castro_amd_new_sponge_source_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, C.POINTER(Sponge), C.POINTER(Geom),
                                                       C.POINTER(Params), C.c_double, C.c_void_p]
        L.castro_amd_sources_mf_opts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(SourceBox), C.POINTER(SourceOpts),
                                                 C.POINTER(Geom), C.POINTER(Params), C.c_double, C.c_int, C.c_void_p]
    if hasattr(L, "castro_amd_add_pointmass_mf"):           # absent from A/B builds of revisions before the point mass
        PP = C.POINTER(PointMassParams)
        L.castro_amd_add_pointmass_fab.argtypes = [C.c_void_p, PF, PP, C.POINTER(Geom), C.c_void_p, C.c_void_p]
        L.castro_amd_add_pointmass_mf.argtypes = [C.c_void_p, C.c_int, PF, PP, C.POINTER(Geom), C.c_void_p, C.c_void_p]
        L.castro_amd_pointmass_delta_mf.argtypes = [C.c_void_p, C.c_int, C.POINTER(PointMassBox), PP, C.POINTER(Geom), C.c_void_p,
                                                    C.c_void_p]
        L.castro_amd_pointmass_apply_mf.argtypes = [C.c_void_p, C.c_int, C.POINTER(PointMassBox), PP, C.POINTER(Geom), C.c_void_p,
                                                    C.c_void_p, C.c_void_p]
    if hasattr(L, "castro_amd_tracer_locate"):              # absent from A/B builds of revisions before the tracer particles
        PT, PB = C.POINTER(Tracers), C.POINTER(TracerBox)
        L.castro_amd_tracer_advect_mf.argtypes = [C.c_void_p, C.c_int, C.c_int, PB, C.POINTER(Geom), C.c_double, C.c_int, PT,
                                                  C.c_void_p, C.c_void_p]
        L.castro_amd_tracer_locate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), PB,
                                               C.POINTER(Geom), PT, C.c_void_p, C.c_void_p]
        L.castro_amd_tracer_sample_mf.argtypes = [C.c_void_p, C.c_int, C.c_int, PB, C.POINTER(Geom), C.c_int, C.POINTER(C.c_int), PT,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
        L.castro_amd_tracer_count_mf.argtypes = [C.c_void_p, C.c_int, C.c_int, PB, C.POINTER(Geom), PT, C.c_void_p]
    if hasattr(L, "castro_amd_tracer_unpack"):              # absent from A/B builds of revisions before the migration
        PT = C.POINTER(Tracers)
        L.castro_amd_tracer_migrate_count.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                                                      PT, C.c_void_p, C.c_void_p, C.c_void_p]
        L.castro_amd_tracer_migrate_pack.argtypes = [C.c_void_p, C.c_int, C.c_int, PT, C.c_void_p, PT, C.c_void_p, C.c_longlong,
                                                     C.c_void_p]
        L.castro_amd_tracer_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, PT, C.c_longlong, C.c_void_p]
    if hasattr(L, "castro_amd_fab_pack"):                   # absent from A/B builds of revisions before checkpoints
        L.castro_amd_fab_pack.argtypes = [C.c_void_p, C.c_int, C.POINTER(PackEntry), C.c_void_p, C.c_void_p, C.c_void_p]
        L.castro_amd_fab_unpack.argtypes = [C.c_void_p, C.c_int, C.POINTER(PackEntry), C.c_void_p, C.c_void_p]
    if hasattr(L, "castro_amd_poisson_solve"):              # absent from A/B builds of revisions before Poisson gravity
        PMP = C.POINTER(Multipole)
        L.castro_amd_multipole_moments_mf.argtypes = [C.c_void_p, C.c_int, C.POINTER(DiagBox), C.POINTER(Geom), PMP, C.c_void_p,
                                                      C.c_void_p]
        L.castro_amd_multipole_phi_bc_fab.argtypes = [C.c_void_p, PF, C.POINTER(Geom), PMP, C.c_void_p, C.c_void_p]
        L.castro_amd_poisson_plan_create.argtypes = [C.c_void_p, C.POINTER(Geom), C.POINTER(C.c_void_p)]
        L.castro_amd_poisson_plan_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.castro_amd_poisson_plan_destroy.restype = None
        L.castro_amd_poisson_solve.argtypes = [C.c_void_p, C.c_void_p, PF, PF, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                               C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        L.castro_amd_poisson_level_op.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, PF, PF, PF, C.c_void_p, C.c_void_p]
        L.castro_amd_grad_phi_to_grav_fab.argtypes = [C.c_void_p, PF, PF, C.POINTER(Geom), C.c_void_p]
    if hasattr(L, "castro_amd_poisson_cf_bc_fab"):          # absent from A/B builds of revisions before the level solves
        L.castro_amd_poisson_cf_bc_fab.argtypes = [C.c_void_p, PF, I3, I3, PF, PF, C.c_double, C.c_void_p]
    if hasattr(L, "castro_amd_poisson_boxes_solve"):        # absent from A/B builds of revisions before levels of several boxes
        PI = C.POINTER(C.c_int)
        L.castro_amd_poisson_boxes_plan_create.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, PI, PI, C.POINTER(C.c_void_p)]
        L.castro_amd_poisson_boxes_cf_bc.argtypes = [C.c_void_p, C.c_void_p, PF, PF, PF, C.c_double, C.c_void_p]
        L.castro_amd_poisson_boxes_solve.argtypes = [C.c_void_p, C.c_void_p, PF, PF, C.c_int, PF, C.c_int, C.c_double, C.c_double,
                                                     C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]
        L.castro_amd_grad_phi_to_grav_boxes.argtypes = [C.c_void_p, C.c_void_p, PF, PF, C.c_int, PF, C.c_void_p]
        L.castro_amd_poisson_boxes_level_op.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, PF, PF, PF, PF, C.c_void_p,
                                                        C.c_void_p]
    L.castro_amd_step_control.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_double, C.c_double,
                                          C.c_double, C.c_int, C.c_void_p]
    L.castro_amd_clean_state_fab.argtypes = [C.c_void_p, PF, I3, I3, C.POINTER(Params), C.c_int, C.c_void_p]
    L.castro_amd_clean_state_reduce_fab.argtypes = [C.c_void_p, PF, I3, I3, C.POINTER(Geom), C.POINTER(Params),
                                                    C.c_int, C.c_void_p, C.c_void_p]
    L.castro_amd_estdt_fab.argtypes = [C.c_void_p, PF, I3, I3, C.POINTER(Geom), C.POINTER(Params),
                                       C.c_void_p, C.c_void_p]
    L.castro_amd_derive_fab.argtypes = [C.c_void_p, C.c_int, PF, PF, C.c_int, I3, I3, C.POINTER(Geom), C.POINTER(Params),
                                        C.POINTER(C.c_double * 3), C.c_void_p]
    D3 = C.POINTER(C.c_double * 3)
    L.castro_amd_old_gravity_source_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, D3, C.c_int, C.c_double, C.c_void_p]
    L.castro_amd_new_gravity_source_fab.argtypes = [C.c_void_p, PF, PF, PF, PF, I3, I3, D3, C.c_int, C.c_double,
                                                    C.POINTER(Geom), C.c_void_p]
    L.castro_amd_old_rotation_source_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, C.POINTER(Rotation), C.POINTER(Geom),
                                                     C.c_double, C.c_void_p]
    L.castro_amd_new_rotation_source_fab.argtypes = [C.c_void_p, PF, PF, PF, PF, I3, I3, C.POINTER(Rotation), C.POINTER(Geom),
                                                     C.c_double, C.c_void_p]
    L.castro_amd_saxpy_fab.argtypes = [C.c_void_p, PF, C.c_double, PF, C.c_int, I3, I3, C.c_void_p]
    L.castro_amd_error_tag_fab.argtypes = [C.c_void_p, PF, C.c_int, PF, I3, I3, C.c_int, C.c_double, C.c_void_p]
    L.castro_amd_fab_ops.argtypes = [C.c_void_p, C.c_int, C.POINTER(FabOp), C.c_void_p]
    L.castro_amd_apply_source_fab.argtypes = [C.c_void_p, PF, PF, C.c_double, PF, C.c_int, I3, I3, C.POINTER(Params), C.c_int, C.c_void_p]
    L.castro_amd_cc_interp_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, C.c_int, C.c_void_p]
    L.castro_amd_fillpatch_shell_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, C.c_int, C.POINTER(Params), C.c_int, C.c_void_p]
    L.castro_amd_lincomb_fab.argtypes = [C.c_void_p, PF, C.c_double, PF, C.c_double, PF, C.c_int, I3, I3, C.c_void_p]
    L.castro_amd_avgdown_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, C.c_int, C.c_void_p]
    L.castro_amd_fluxreg_crse_init_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, C.c_int, C.c_double, C.c_void_p]
    L.castro_amd_fluxreg_fine_add_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, C.c_int, C.c_int, C.c_double, C.c_void_p]
    L.castro_amd_reflux_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]
    if hasattr(L, "castro_amd_fluxreg_to_flux_fab"):        # absent from A/B builds of revisions before update_sources_after_reflux
        L.castro_amd_fluxreg_to_flux_fab.restype = C.c_int
        L.castro_amd_fluxreg_to_flux_fab.argtypes = [C.c_void_p, PF, PF, PF, I3, I3, C.c_int, C.c_void_p]
    L.castro_amd_bc_fill_fab.argtypes = [C.c_void_p, PF, C.POINTER(Geom), C.c_void_p]
    if hasattr(L, "castro_amd_ext_bc_fill_fab"):            # absent from A/B builds of revisions before the boundary overrides
        L.castro_amd_ext_bc_fill_fab.argtypes = [C.c_void_p, PF, C.POINTER(Geom), C.POINTER(Params), C.POINTER(ExtBc), C.c_void_p,
                                                 C.c_void_p]
    L.castro_amd_copy_fab.argtypes = [C.c_void_p, PF, PF, I3, I3, C.c_void_p]
    L.castro_amd_pack_fab.argtypes = [C.c_void_p, PF, I3, I3, C.c_void_p, C.c_void_p]
    L.castro_amd_unpack_fab.argtypes = [C.c_void_p, PF, I3, I3, C.c_void_p, C.c_void_p]
    for f in (L.castro_amd_pack_regions_fab, L.castro_amd_unpack_regions_fab):
        f.argtypes = [C.c_void_p, PF, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.c_void_p, C.c_void_p]
    L.castro_amd_sedov_init_fab.argtypes = [C.c_void_p, PF, I3, I3, C.POINTER(Geom), C.POINTER(Params),
                                            C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
    L.castro_amd_sod_init_fab.argtypes = [C.c_void_p, PF, I3, I3, C.POINTER(Geom), C.POINTER(Params)] + \
        [C.c_double] * 6 + [C.c_int, C.c_double, C.c_void_p]
    if hasattr(L, "castro_amd_comm_version"):               # absent from A/B builds of revisions before the C-level halo exchange
        L.castro_amd_comm_version.restype = C.c_char_p
        L.castro_amd_comm_unique_id.argtypes = [C.c_void_p]
        L.castro_amd_comm_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.castro_amd_comm_adopt.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int]
        L.castro_amd_comm_rank.argtypes = [C.c_void_p]
        L.castro_amd_comm_size.argtypes = [C.c_void_p]
        L.castro_amd_comm_destroy.argtypes = [C.c_void_p]
        L.castro_amd_halo_plan_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.POINTER(HaloRegion), C.c_int]
        L.castro_amd_halo_plan_destroy.argtypes = [C.c_void_p]
        L.castro_amd_halo_plan_bytes_sent.argtypes = [C.c_void_p]
        L.castro_amd_halo_plan_bytes_sent.restype = C.c_longlong
        L.castro_amd_fill_boundary.argtypes = [C.c_void_p, C.c_void_p, PF, C.POINTER(Geom), C.c_void_p]
        L.castro_amd_fill_boundary_ex.argtypes = [C.c_void_p, C.c_void_p, PF, C.POINTER(Geom), C.c_int, C.c_void_p]
        L.castro_amd_halo_plan_wait_packed.argtypes = [C.c_void_p, C.c_void_p]
        L.castro_amd_halo_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.POINTER(HaloMsg), C.c_int,
                                                   C.POINTER(HaloMsg), C.c_int]
        L.castro_amd_halo_group_destroy.argtypes = [C.c_void_p]
        L.castro_amd_halo_group_bytes_sent.argtypes = [C.c_void_p]
        L.castro_amd_halo_group_bytes_sent.restype = C.c_longlong
        L.castro_amd_fill_boundary_group.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Fab), C.POINTER(Geom), C.c_void_p]
        L.castro_amd_fill_boundary_group_ex.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Fab), C.POINTER(Geom), C.c_int, C.c_void_p]
        L.castro_amd_halo_group_wait_packed.argtypes = [C.c_void_p, C.c_void_p]
        L.castro_amd_allreduce_min.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.castro_amd_ctx_profile.argtypes = [C.c_void_p, C.c_int]
    L.castro_amd_ctx_profile_count.argtypes = [C.c_void_p]
    L.castro_amd_ctx_profile_get.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int,
                                             C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.castro_amd_ctx_profile_reset.argtypes = [C.c_void_p]
    L.castro_amd_berger_rigoutsos.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int]
    V = C.c_void_p
    L.castro_amd_cmpflx_points.argtypes = [C.c_longlong, C.c_int, V, V, V, V, V, V, C.POINTER(Params), V, V]
    L.castro_amd_ppm_points.argtypes = [C.c_longlong, V, V, V, V, C.c_double, V, V]
    L.castro_amd_flatten_points.argtypes = [C.c_longlong, V, V, V, V]
    L.castro_amd_trans_points.argtypes = [C.c_longlong, C.c_int, C.c_int, V, V, V, V, V, V, C.c_double, C.c_double,
                                          C.POINTER(Params), V, V]
    _libs[mode] = L
    return L


def i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


def default_params(**overrides):
    """castro_amd_params with the reference defaults for the Sedov setup; keyword overrides are applied
    and the derived floors recomputed (Castro_setup.cpp:222-288)."""
    p = Params()
    load().castro_amd_default_params(C.byref(p))
    if overrides:
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise AttributeError("castro_amd_params has no field %r" % k)
            setattr(p, k, v)
        if any(k in overrides for k in ("eos_gamma", "small_dens", "small_temp", "abar")):
            if "small_pres" not in overrides:
                p.small_pres = 1.e-100
            if "small_ener" not in overrides:
                p.small_ener = 1.e-100
            load().castro_amd_finalize_params(C.byref(p))
    return p


def make_geom(n_cell, prob_lo=(0., 0., 0.), prob_hi=(1., 1., 1.), lo_bc=(2, 2, 2), hi_bc=(2, 2, 2),
              domlo=(0, 0, 0)):
    g = Geom()
    for d in range(3):
        g.problo[d] = prob_lo[d]
        g.probhi[d] = prob_hi[d]
        g.dx[d] = (prob_hi[d] - prob_lo[d]) / n_cell[d]
        g.domlo[d] = domlo[d]
        g.domhi[d] = domlo[d] + n_cell[d] - 1
        g.lo_bc[d] = lo_bc[d]
        g.hi_bc[d] = hi_bc[d]
    g.coord = 0
    return g


_I3 = C.c_int * 3


def fab_desc(ptr, lo, hi, ncomp):
    return Fab(ptr, _I3(int(lo[0]), int(lo[1]), int(lo[2])), _I3(int(hi[0]), int(hi[1]), int(hi[2])), int(ncomp))


_FAB_MEMO = {}


def fab_of(tensor, lo, hi):
    """Descriptor for a contiguous torch tensor shaped (ncomp, nz, ny, nx) covering box [lo, hi]
    (C order of that shape == AMReX FAB layout: i fastest, component slowest).  A descriptor is a function of
    (pointer, shape, box) only, so it is memoised: a level of small AMR boxes builds thousands per coarse step."""
    if tensor is None:
        return fab_desc(None, lo, hi, 0)
    shp = tensor.shape
    key = (tensor.data_ptr(), shp, lo if type(lo) is tuple else tuple(lo), hi if type(hi) is tuple else tuple(hi))
    f = _FAB_MEMO.get(key)
    if f is not None and tensor.is_contiguous():
        return f
    if not (tensor.is_contiguous() and shp[-1] == hi[0] - lo[0] + 1 and shp[-2] == hi[1] - lo[1] + 1 and shp[-3] == hi[2] - lo[2] + 1):
        raise AssertionError("FAB tensors must be contiguous and shaped (ncomp, nz, ny, nx) of their box: %s for %s"
                             % (tuple(shp), (lo, hi)))
    f = fab_desc(key[0], lo, hi, shp[0] if len(shp) == 4 else 1)
    if len(_FAB_MEMO) > 4096:
        _FAB_MEMO.clear()
    _FAB_MEMO[key] = f
    return f


def check(rc, what):
    if rc != OK:
        names = {ERR_ARG: "bad argument", ERR_UNSUPPORTED: "unsupported option", ERR_NOMEM: "out of device memory",
                 ERR_HIP: "HIP runtime error / no device"}
        raise RuntimeError("castro_amd: %s failed: %s (%d)" % (what, names.get(rc, "error"), rc))

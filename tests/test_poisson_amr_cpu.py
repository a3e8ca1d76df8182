"""CPU tests of Poisson gravity on the levels of CastroAmr (level solves: gravity.no_sync = 1, gravity.no_composite = 1): the
acceptance and the refusals of CastroAmr(gravity=PoissonGravity(...)), the restatement of the coarse-fine boundary potential
(tests/poisson_amr_ref.py) on a linear field, the gain of a refined patch over the coarse solve, and the driver on
PoissonAmrOracleBackend."""
import numpy as np
import pytest

from tests import poisson_amr_ref as A
from tests import poisson_ref as R

_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _amr(oracle, **kw):
    import castro_amd
    kw.setdefault("gravity", castro_amd.PoissonGravity())
    kw.setdefault("do_grav", True)
    kw.setdefault("make_hydro", lambda: A.PoissonAmrOracleBackend())
    if "patches" not in kw and "refine" not in kw:
        kw.setdefault("patch_crse", A.PATCH1)
    return castro_amd.CastroAmr((16, 16, 16), params=oracle.default_params(**R.DUST_PARAMS), **kw)


# ---- 1. acceptance and refusals --------------------------------------------------------------------------------------------------
def test_poisson_gravity_is_accepted_on_a_hierarchy(oracle):
    import castro_amd
    a = _amr(oracle)
    assert isinstance(a.gravity, castro_amd.PoissonGravity) and len(a.lev) == 2
    assert a.gravity.solves(1) and castro_amd.PoissonGravity(max_solve_level=0).solves(0)
    assert not castro_amd.PoissonGravity(max_solve_level=0).solves(1)
    a.close()


def test_refusals(oracle):
    import castro_amd
    from castro_amd import _lib
    PG = castro_amd.PoissonGravity
    with pytest.raises(NotImplementedError, match="single level only"):
        _amr(oracle, gravity=None, poisson=PG())                       # the poisson= keyword keeps its refusal
    with pytest.raises(TypeError, match="MonopoleGravity or a castro_amd.PoissonGravity"):
        _amr(oracle, gravity="poisson")

    class TwoRanks:
        rank, size = 0, 2
    with pytest.raises(NotImplementedError, match="more than one rank"):
        _amr(oracle, comm=TwoRanks())
    with pytest.raises(NotImplementedError, match="base_grid"):
        _amr(oracle, base_grid=(2, 1, 1))
    with pytest.raises(NotImplementedError, match="level 1 would have 2 boxes"):
        _amr(oracle, patch_crse=None, patches=[[((2, 2, 2), (5, 5, 5)), ((8, 8, 8), (11, 11, 11))]])
    with pytest.raises(NotImplementedError, match="touches the domain boundary"):
        _amr(oracle, patch_crse=((0, 4, 4), (7, 11, 11)))
    with pytest.raises(NotImplementedError, match="touches the domain boundary"):
        _amr(oracle, patch_crse=((4, 4, 8), (11, 11, 15)))
    for kw in (dict(no_sync=False), dict(no_composite=False)):
        with pytest.raises(NotImplementedError, match="composite"):
            PG(**kw)
    with pytest.raises(NotImplementedError, match="periodic face"):
        _amr(oracle, lo_bc=(0, 2, 2), hi_bc=(0, 2, 2))
    with pytest.raises(NotImplementedError, match="Symmetry face"):
        _amr(oracle, lo_bc=(3, 2, 2))
    with pytest.raises(NotImplementedError, match="use_point_mass with Poisson gravity"):
        _amr(oracle, use_point_mass=True, point_mass=1.0)
    with pytest.raises(NotImplementedError, match="check_int with Poisson gravity"):
        _amr(oracle, check_int=2)
    a = _amr(oracle)
    with pytest.raises(NotImplementedError, match="writeCheckpoint with Poisson gravity"):
        a.writeCheckpoint("never_written")
    with pytest.raises(NotImplementedError, match="restart with Poisson gravity"):
        a.restart("never_read")
    with pytest.raises(ValueError, match="belongs to one"):
        _amr(oracle, gravity=a.gravity)
    with pytest.raises(ValueError, match="needs do_grav=True"):
        _amr(oracle, do_grav=False)
    with pytest.raises(ValueError, match="not together with diffusion"):
        _amr(oracle, diffusion=_lib.make_diffusion(1.0))
    # a level-2 box whose coarsened box, grown by one, leaves the valid box of level 1 (fine zones 8..23)
    with pytest.raises(ValueError, match="does not lie inside the valid box"):
        _amr(oracle, patch_crse=None, patches=[A.PATCH1, ((8, 12, 12), (15, 19, 19))])
    with pytest.raises(ValueError, match="max_solve_level must not be negative"):
        PG(max_solve_level=-1)
    with pytest.raises(RuntimeError, match="needs CastroAmr"):
        castro_amd.CastroAmr((16, 16, 16), params=oracle.default_params(), make_hydro=lambda: A.PoissonAmrOracleBackend(),
                             patch_crse=A.PATCH1).phi_grav(0)


def test_hse_faces_are_refused(oracle):
    from castro_amd import _lib
    ext = _lib.make_ext_bc(zl="hse", hse_zero_vels=1)
    geom = _lib.make_geom((16, 16, 16), lo_bc=(2, 2, 1), hi_bc=(2, 2, 2))
    if not _lib.ext_bc_hse_faces(ext, geom):
        pytest.fail("the case has no HSE face")
    with pytest.raises(ValueError, match="HSE boundaries assume constant gravity"):
        _amr(oracle, lo_bc=(2, 2, 1), ext_bc=ext)


def test_a_box_the_bottom_solver_cannot_take_is_named(oracle):
    """a box of 34 zones a side coarsens once, to 17^3 = 4913 zones, more than CASTRO_AMD_POISSON_MAX_BOTTOM = 4096: ValueError with
    the level and the box; 32 zones a side coarsen to 2^3 and pass"""
    import castro_amd
    from castro_amd import _lib
    g = castro_amd.PoissonGravity()
    g.amr = type("H", (), {"n_cell": (256, 256, 256)})()
    with pytest.raises(ValueError, match=r"level 1 .*CASTRO_AMD_POISSON_MAX_BOTTOM.*blocking_factor"):
        g._check_bottom(1, ((2, 2, 2), (35, 35, 35)), (34, 34, 34))
    assert _lib.poisson_level_extents((34, 34, 34))[-1] == (17, 17, 17)
    g._check_bottom(1, ((0, 0, 0), (31, 31, 31)), (32, 32, 32))


# ---- 2. exactness on a linear field ----------------------------------------------------------------------------------------------
CX, CY, CZ, CT, C0 = 2.0, -3.0, 1.5, 0.75, 0.25                 # phi = C0 + CX x + CY y + CZ z + CT t on the unit cube, t in [0, 1]
LIN_PATCHES = [((4, 4, 4), (11, 11, 11)), ((2, 4, 6), (5, 11, 13))]


def _linear(box, h, t, dtype=np.float64, face_shell_of=None):
    """the field at the zone centres of `box` (zones of width h); face_shell_of = (lo, hi): at the centres of the zones of that
    box grown by one, the coordinate of a direction in which a zone lies outside moved onto the face"""
    ax = []
    for d in range(3):
        i = np.arange(box[0][d], box[1][d] + 1)
        x = (i.astype(dtype) + dtype(0.5)) * dtype(h)
        if face_shell_of is not None:
            lo, hi = face_shell_of
            x = np.where(i < lo[d], dtype(lo[d]) * dtype(h), np.where(i > hi[d], dtype(hi[d] + 1) * dtype(h), x))
        sh = [1, 1, 1]
        sh[2 - d] = len(i)
        ax.append(x.reshape(sh))
    return dtype(C0) + dtype(CX) * ax[0] + dtype(CY) * ax[1] + dtype(CZ) * ax[2] + dtype(CT) * dtype(t)


@pytest.mark.parametrize("a", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("patch", LIN_PATCHES)
def test_face_values_and_patch_solve_of_a_linear_field(a, patch):
    """Coarse phi linear in space and time on 16^3 zones of the unit cube, zero density.  (i) The face values equal the field on the
    face within CF_ROUNDINGS = 39 roundings (the count is derived in poisson_amr_ref's docstring) x 2^-53 x the sum of the
    magnitudes of the terms; the field itself is evaluated in extended precision.  (ii) The solve of the patch returns the field:
    with A the operator, A (phi - u) = r(u) - r(phi) for the residuals of the solution and of the field u with the same ghost
    values, and |A^-1|_inf <= L^2 / 6 (w = x (L - x) / 2 along the shortest side L is a discrete supersolution: -lap_h w = 1 inside
    and 3/4 in a boundary zone, whose ghost 2 * 0 - w_in lies h^2 / 4 above the parabola), so
    |phi - u| <= L^2 / 6 * (|r(phi)| + |r(u)| + 2 gamma), gamma = 16 * 2^-52 * max(sum |stencil terms|) for evaluating a residual
    (the gamma of poisson_ref.dense_check).  With zero density the stopping tolerance is zero: the solve runs its V-cycles down to
    rounding and is judged by the residual it reports."""
    hc, hf = 1.0 / 16, 1.0 / 32
    cbox = ((-1, -1, -1), (16, 16, 16))
    old, new = _linear(cbox, hc, 0.0), _linear(cbox, hc, 1.0)
    flo, fhi = tuple(2 * x for x in patch[0]), tuple(2 * x + 1 for x in patch[1])
    n = tuple(fhi[d] - flo[d] + 1 for d in range(3))
    got = A.face_values(old, cbox, new, cbox, flo, fhi, a)
    mag = A.face_values(old, cbox, new, cbox, flo, fhi, a, mag=True)
    LD = np.longdouble
    pbox = (tuple(x - 1 for x in flo), tuple(x + 1 for x in fhi))
    exact = _linear(pbox, hf, LD(a), dtype=LD, face_shell_of=(flo, fhi))
    face = ~np.isnan(got) & (mag > 0.0)
    assert face.sum() == 2 * (n[0] * n[1] + n[0] * n[2] + n[1] * n[2])
    err = np.abs(got.astype(LD) - exact)[face]
    bound = A.CF_ROUNDINGS * A.U53 * mag[face]
    print("linear field, a = %g, patch %s: worst face deviation / allowance = %.3g" % (a, patch, float((err / bound).max())))
    assert np.all(err <= bound)
    edges = ~np.isnan(got) & ~face
    assert edges.sum() == 4 * (n[0] + n[1] + n[2]) + 8 and np.all(got[edges] == 0.0)
    # (ii) the solve of the patch from zero
    phi = np.zeros(got.shape)
    A.cf_bc(phi, pbox, flo, fhi, old, cbox, new, cbox, a)
    assert np.array_equal(_bits(phi[~np.isnan(got)]), _bits(got[~np.isnan(got)])) and np.all(phi[1:-1, 1:-1, 1:-1] == 0.0)
    dx = (hf, hf, hf)
    cycles, ok, rnorm, hist = R.solve(n, dx, phi, np.zeros(n[::-1]), 4.0 * np.pi)
    assert hist[0] == 0.0 and hist[2] > 0.0
    u = phi.copy()
    u[1:-1, 1:-1, 1:-1] = _linear((flo, fhi), hf, LD(a), dtype=LD).astype(np.float64)
    L0 = R.levels(n, dx)[0]
    smag = np.zeros(L0.shape)
    r_phi = np.abs(R.residual(L0, phi, np.zeros(L0.shape), smag)).max()
    gamma = 16.0 * R.U52 * smag.max()
    r_u = np.abs(R.residual(L0, u, np.zeros(L0.shape))).max()
    Lmin = min(n) * hf
    dev = np.abs(phi - u)[1:-1, 1:-1, 1:-1].max()
    bound = Lmin * Lmin / 6.0 * (r_phi + r_u + 2.0 * gamma)
    print("patch solve: %d cycles, reported norm %.3g, |phi - u| = %.3g, bound %.3g" % (cycles, rnorm, dev, bound))
    assert rnorm == r_phi and rnorm <= 1e-10 * hist[2]
    assert dev <= bound


# ---- 3. refinement must help -----------------------------------------------------------------------------------------------------
def _sphere(n):
    h = 1.0 / n
    x = (np.arange(n) + 0.5) * h - 0.5
    r = np.sqrt(x[None, None, :] ** 2 + x[None, :, None] ** 2 + x[:, None, None] ** 2)
    return 0.5 * (1.0 - np.tanh((r - 0.2) / 0.02))


def _monopole_solve(n, oracle):
    """the single-level solve on n^3 zones of the unit cube, G = 1, monopole boundary values: (phi with its ghost shell, g)"""
    from castro_amd import _lib
    geom = _lib.make_geom((n, n, n))
    mp = _lib.make_multipole(geom, (0.5, 0.5, 0.5), 0, 1.0)
    rho = _sphere(n)
    q, _ = R.moments([(rho, (0, 0, 0), None)], geom, mp)
    phi = np.zeros((n + 2,) * 3)
    R.phi_bc(q, geom, mp, phi, ((-1, -1, -1), (n, n, n)))
    dx = tuple(geom.dx[d] for d in range(3))
    out = R.solve((n, n, n), dx, phi, rho, 4.0 * np.pi)
    assert out[1]
    return phi, R.grad_phi(phi, dx), rho


def test_refinement_must_help(oracle):
    """Base 16^3 on the unit cube, 4 pi G = 4 pi, a smoothed sphere of radius 0.2, monopole boundary values; the patch: coarse
    (4..11)^3 -> 16^3 fine zones with its own density and Dirichlet data from the coarse solve.  Against the uniform 32^3 solve on
    the zones of the patch, the patch solve must be closer than HALF the deviation of the coarse solution injected onto the fine
    zones (piecewise constant), in phi and in g_x.  A condition, not a tolerance."""
    pc, gc, _ = _monopole_solve(16, oracle)
    pf, gf, rho32 = _monopole_solve(32, oracle)
    flo, fhi = (8, 8, 8), (23, 23, 23)
    cbox = ((-1, -1, -1), (16, 16, 16))
    phi = np.zeros((18, 18, 18))
    pbox = ((7, 7, 7), (24, 24, 24))
    A.cf_bc(phi, pbox, flo, fhi, pc, cbox, pc, cbox, 1.0)
    dx = (1.0 / 32,) * 3
    out = R.solve((16, 16, 16), dx, phi, rho32[8:24, 8:24, 8:24], 4.0 * np.pi)
    assert out[1], out
    gp = R.grad_phi(phi, dx)
    up = lambda x: np.repeat(np.repeat(np.repeat(x, 2, axis=-3), 2, axis=-2), 2, axis=-1)
    want_phi, want_g = pf[9:25, 9:25, 9:25], gf[0][8:24, 8:24, 8:24]
    inj_phi, inj_g = up(pc[5:13, 5:13, 5:13]), up(gc[0][4:12, 4:12, 4:12])
    e_phi, e_inj = np.abs(phi[1:-1, 1:-1, 1:-1] - want_phi).max(), np.abs(inj_phi - want_phi).max()
    g_phi, g_inj = np.abs(gp[0] - want_g).max(), np.abs(inj_g - want_g).max()
    print("phi: patch %.3g against injected %.3g (ratio %.3f); g_x: patch %.3g against injected %.3g (ratio %.3f)"
          % (e_phi, e_inj, e_phi / e_inj, g_phi, g_inj, g_phi / g_inj))
    assert e_phi < 0.5 * e_inj
    assert g_phi < 0.5 * g_inj


# ---- 4. the driver on the CPU backend --------------------------------------------------------------------------------------------
def _run(oracle, case, **kw):
    key = (case,) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        _CACHE[key] = A.dust_amr_run(lambda: A.PoissonAmrOracleBackend(), oracle.default_params(**R.DUST_PARAMS), case, **kw)
    return _CACHE[key]


def _pattern(nlev, l=0, a=0.0, out=None):
    """the (level, old / new, a) solves of one coarse step of a subcycled hierarchy"""
    out = [] if out is None else out
    out.append((l, "old", a))
    out.append((l, "new", a + 0.5 if l > 0 else 1.0))
    if l + 1 < nlev:
        _pattern(nlev, l + 1, 0.0, out)
        _pattern(nlev, l + 1, 0.5, out)
    return out


def _same_solves(log, want):
    """the same levels and time levels in the same order; a is the fraction _Level forms for fill_grav (alpha + dt / dt_parent, a
    quotient of host doubles): equal to the pattern's within a few roundings"""
    assert [x[:2] for x in log] == [x[:2] for x in want], (log, want)
    assert all(abs(x[2] - w[2]) <= 4.0 * R.U52 for x, w in zip(log, want)), (log, want)


@pytest.mark.parametrize("case", ["one", "two"])
def test_driver_solve_sequence_and_first_solve(oracle, case):
    import castro_amd
    a, dts = _run(oracle, case)
    nlev = len(A.CASES[case]) + 1
    assert len(a.lev) == nlev and all(d > 0.0 for d in dts)
    want = _pattern(nlev) * A.AMR_STEPS
    _same_solves(a.gravity.solve_log, want)
    assert [x for x in want if x[0] == 1][:4] == [(1, "old", 0.0), (1, "new", 0.5), (1, "old", 0.5), (1, "new", 1.0)]
    for l in range(nlev):
        st = a.poisson_stats(l)
        phi, g = a.phi_grav(l).numpy(), a.lev[l].boxes[0].grav_new.numpy()
        assert np.isfinite(phi).all() and np.isfinite(g).all() and np.all(phi[0, 1:-1, 1:-1, 1:-1] < 0.0)
        assert st["first"]["cycles"] >= st["new"]["cycles"] >= 0
        if l > 0:
            assert phi[0, 0, 0, 0] == 0.0 and phi[0, 0, 0, 5] == 0.0, "corners and edges of the ghost shell of a level that solves"
    # the first level-0 solve has the bits of the single-level driver's first solve on the same state
    b = castro_amd.CastroAmr(A.AMR_N, params=oracle.default_params(**R.DUST_PARAMS), make_hydro=lambda: A.PoissonAmrOracleBackend(),
                             do_grav=True, gravity=castro_amd.PoissonGravity(center=R.DUST_CENTER), patches=A.CASES[case], **R.DUST_GEOM)
    b.initData("dust_collapse", **R.DUST_PROB)
    c = castro_amd.Castro(A.AMR_N, params=oracle.default_params(**R.DUST_PARAMS), hydro=A.PoissonAmrOracleBackend(), do_grav=True,
                          poisson=castro_amd.PoissonGravity(), **R.DUST_GEOM)
    c.center = R.DUST_CENTER
    c.initData("dust_collapse", **R.DUST_PROB)
    c.S_new_b.copy_(b.lev[0].boxes[0].S_new_b)
    c.step()
    first, single = a.poisson_stats(0)["first"], c.poisson_stats()["first"]
    assert first["cycles"] == single["cycles"] > 0
    assert np.array_equal(_bits(np.array(first["history"])), _bits(np.array(single["history"])))


def test_max_solve_level_zero_is_fill_coarse_patch(oracle):
    """max_solve_level = 0: the fine level makes no solve; its phi and g -- whole FABs, ghost zones included -- are the time
    combination and cc_interp of level 0, bit for bit"""
    import torch
    a, _ = _run(oracle, "one", max_solve_level=0)
    assert all(l == 0 for l, _, _ in a.gravity.solve_log) and len(a.gravity.solve_log) == 2 * A.AMR_STEPS
    assert a.poisson_stats(1) == {"first": None, "old": None, "new": None}
    be = A.PoissonAmrOracleBackend()
    P = a.gravity._lev[0]
    c, f = a.lev[0].boxes[0], a.lev[1].boxes[0]
    for which, al in (("old", 0.5), ("new", 1.0)):                      # the last advance of the fine level
        phi = a.phi_grav(1, new=which == "new")
        want = torch.full_like(phi, float("nan"))
        pbox = a.gravity._lev[1]["phibox"]
        A.fill_coarse_patch(be, P["phi_old"], P["phi_new"], P["phibox"], want, pbox, al, 1)
        assert np.array_equal(_bits(phi.numpy()), _bits(want.numpy())), which
        g = getattr(f, "grav_" + which)
        wg = torch.full_like(g, float("nan"))
        A.fill_coarse_patch(be, c.grav_old, c.grav_new, c.gravbox, wg, f.gravbox, al, 3)
        assert np.array_equal(_bits(g.numpy()), _bits(wg.numpy())), which
    # and the run differs from the one whose fine level solves
    b, _ = _run(oracle, "one")
    assert not np.array_equal(b.lev[1].boxes[0].grav_new.numpy(), f.grav_new.numpy())


def test_update_sources_after_reflux_runs(oracle):
    a, dts = _run(oracle, "one", update_sources_after_reflux=True)
    assert all(d > 0.0 for d in dts) and np.isfinite(a.lev[1].boxes[0].S_new().numpy()).all()
    _same_solves(a.gravity.solve_log, _pattern(2) * A.AMR_STEPS)          # the field is not rebuilt after a reflux


def test_a_regrid_that_moves_the_box_remakes_the_plan(oracle):
    """refine= on a star of radius 2e8 (the density tags are the coarse zones 6..9, buffered and blocked to 4..11): a regrid with a
    wider buffer makes the level-1 box 2..13 -- 24^3 fine zones, a plan of other extents"""
    import castro_amd
    g = castro_amd.PoissonGravity(center=R.DUST_CENTER)
    a = castro_amd.CastroAmr(A.AMR_N, params=oracle.default_params(**R.DUST_PARAMS), make_hydro=lambda: A.PoissonAmrOracleBackend(),
                             do_grav=True, gravity=g, refine=[("density", "value_greater", 5.e8)], regrid_int=2, max_level=1,
                             blocking_factor=4, **R.DUST_GEOM)
    a.initData("dust_collapse", **dict(R.DUST_PROB, r_0=2.e8))
    assert len(a.lev) == 2 and a.pbox[1] == A.PATCH1
    a.step()
    box0, plan0 = a.lev[1].boxes[0].bx, g._lev[1]["plan"]
    assert g._lev[1]["key"] == box0 and plan0[0] == (16, 16, 16)
    a.n_error_buf = 3
    assert a.regrid(0)
    assert 1 not in g._lev, "the potential and the plan of the level that was re-made are gone"
    assert a.pbox[1] == ((2, 2, 2), (13, 13, 13))
    a.step()
    assert g._lev[1]["key"] == a.lev[1].boxes[0].bx and g._lev[1]["plan"][0] == (24, 24, 24)
    assert np.isfinite(a.phi_grav(1).numpy()).all() and np.isfinite(a.lev[1].boxes[0].S_new().numpy()).all()
    assert a.poisson_stats(1)["first"]["cycles"] > 0
    a.close()
    assert g._lev[1]["plan"] is None and g._lev[0]["plan"] is None
    a.step()
    assert g._lev[1]["plan"] is not None


def test_single_level_and_level_zero_are_one_route(oracle):
    """Castro(poisson=...) and a CastroAmr(gravity=...) with no refined level, two whole steps from the same state: one path, one
    set of bits"""
    A.assert_routes_agree(*A.single_and_hierarchy(lambda: A.PoissonAmrOracleBackend(), oracle.default_params(**R.DUST_PARAMS)))

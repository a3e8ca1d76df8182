"""CPU tests of Poisson gravity on refined levels of SEVERAL boxes: the numpy restatement of the masked passes and of the level's
coarse-fine boundary values (tests/poisson_boxes_ref.py) on its own, and the driver -- CastroAmr(gravity=PoissonGravity(...)) with
patches=[[box, ...]] and with refine= + cluster=True -- on PoissonBoxesOracleBackend."""
import numpy as np
import pytest

from tests import poisson_amr_ref as A
from tests import poisson_boxes_ref as B
from tests import poisson_ref as R

FOURPI = 4.0 * np.pi
ELL_CRSE, NESTED2 = B.ELL_CRSE, B.NESTED2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _amr(oracle, **kw):
    import castro_amd
    kw.setdefault("gravity", castro_amd.PoissonGravity(center=R.DUST_CENTER))
    kw.setdefault("make_hydro", lambda: B.PoissonBoxesOracleBackend())
    return castro_amd.CastroAmr(A.AMR_N, params=oracle.default_params(**R.DUST_PARAMS), do_grav=True, **R.DUST_GEOM, **kw)


# ---- 1. the restatement on its own -----------------------------------------------------------------------------------------------
def test_flags_of_the_ell():
    """the concave corner: the uncovered zone (16, 16, k) is the neighbour of (15, 16, k) across x and of (16, 15, k) across y"""
    plan = B.Plan(B.DX, B.LAYOUTS["ell"])
    assert plan.bb == ((8, 8, 8), (23, 23, 15)) and [L.n for L in plan.lev] == [(16, 16, 8), (8, 8, 4), (4, 4, 2)]
    fl = plan.flags[0]
    assert fl[0, 8, 8] == 0 and fl[3, 8, 7] == B.COVERED | B.face_bit(0, 1) and fl[3, 7, 8] == B.COVERED | B.face_bit(1, 1)
    assert fl[3, 7, 7] == B.COVERED, "a face between two boxes is no boundary"
    assert fl[0, 0, 0] == B.COVERED | B.face_bit(0, 0) | B.face_bit(1, 0) | B.face_bit(2, 0)
    assert int(plan.covered().sum()) == 3 * 512 and int(plan.covered(2).sum()) == 3 * 8
    # unequal alignment: the 4-aligned box stops the coarsening at two levels, the extents (12, 12, 8) would allow three
    un = B.Plan(B.DX, B.LAYOUTS["unequal"])
    assert [L.n for L in un.lev] == [(12, 12, 8), (6, 6, 4), (3, 3, 2)]
    from castro_amd import _lib
    for name, boxes in B.LAYOUTS.items():
        assert [n for _, n in _lib.poisson_boxes_levels(boxes)] == [L.n for L in B.Plan(B.DX, boxes).lev], name
    with pytest.raises(ValueError, match="overlap"):
        B.Plan(B.DX, [B._cube((8, 8, 8)), B._cube((12, 8, 8))])
    with pytest.raises(ValueError, match="refinement"):
        B.Plan(B.DX, [((9, 8, 8), (15, 15, 15))])


def test_cf_values_of_a_linear_field_are_exact():
    """phi linear in x, y, z (in coarse index units, dyadic coefficients: every coarse value is exact) on both time levels: the
    value on every boundary face of the ell is the field at the face centre to CF_ROUNDINGS * 2^-53 * (the magnitudes)"""
    plan = B.Plan(B.DX, B.LAYOUTS["ell"])
    cbox = ((-1, -1, -1), (16, 16, 16))
    ax = [np.arange(-1, 17, dtype=np.float64) + 0.5 for _ in range(3)]
    Z, Y, X_ = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    old = 3.0 + 2.0 * X_ - 5.0 * Y + 0.5 * Z
    new = -1.0 + 0.25 * X_ + 4.0 * Y - 3.0 * Z
    a = 0.25
    shape = (3,) + B.shape_of(plan.facebox)
    got, mag = np.full(shape, np.nan), np.full(shape, np.nan)
    wrote = B.cf_faces(plan, got, old, cbox, new, cbox, a)
    B.cf_faces(plan, mag, old, cbox, new, cbox, a, mag=True)
    assert np.array_equal(wrote, ~np.isnan(got))
    # boundary faces of the ell: 2 x (16 x 8 + 16 x 8) in x and y (the concave corner included), 2 x 192 in z
    assert [int(wrote[d].sum()) for d in range(3)] == [256, 256, 384]
    lo = plan.bb[0]
    n = 0
    for d in range(3):
        kk, jj, ii = np.nonzero(wrote[d])
        pos = [(ii + lo[0] + 0.5) / 2.0, (jj + lo[1] + 0.5) / 2.0, (kk + lo[2] + 0.5) / 2.0]     # fine zone centres, coarse units
        pos[d] = pos[d] - 0.25                                                                  # the low d-face of the zone
        f = lambda c: c[0] + c[1] * pos[0] + c[2] * pos[1] + c[3] * pos[2]
        exact = (1.0 - a) * f((3.0, 2.0, -5.0, 0.5)) + a * f((-1.0, 0.25, 4.0, -3.0))
        err = np.abs(got[d][kk, jj, ii] - exact)
        assert np.all(err <= A.CF_ROUNDINGS * A.U53 * mag[d][kk, jj, ii]), (d, err.max())
        n += len(kk)
    assert n == 896


def _case(name, seed=3):
    boxes = B.LAYOUTS[name]
    plan = B.Plan(B.DX, boxes)
    rng = np.random.default_rng(seed)
    cbox = B.CRSE_BOX.get(name, ((-1, -1, -1), (16, 16, 16)))
    co, cn = rng.normal(size=B.shape_of(cbox)) * 3.0 - 7.0, rng.normal(size=B.shape_of(cbox)) * 3.0 - 7.0
    rho = rng.uniform(0.5, 2.0, size=plan.lev[0].shape)
    start = np.zeros(plan.lev[0].gshape)
    start[1:-1, 1:-1, 1:-1] = rng.normal(size=plan.lev[0].shape) - 7.0
    X = np.zeros((3,) + B.shape_of(plan.facebox))
    B.cf_faces(plan, X, co, cbox, cn, cbox, 0.3)
    return plan, co, cn, cbox, rho, start, X


@pytest.mark.parametrize("name", ["tile2", "tile4"])
def test_masked_solve_of_a_tiling_is_the_one_box_solve(name):
    """a union that tiles its bounding box: the face values are those of cf_bc on the box, and phi, the norm history and the cycle
    count of the masked solve are those of poisson_ref.solve, bit for bit"""
    plan, co, cn, cbox, rho, start, X = _case(name)
    bb, n = plan.bb, plan.lev[0].n
    assert plan.covered().all() and len(plan.lev) == len(R.levels(n, B.DX))
    one = start.copy()
    A.cf_bc(one, plan.phibox, bb[0], bb[1], co, cbox, cn, cbox, 0.3)
    assert np.array_equal(_bits(X[0][:-1, :-1, 0]), _bits(one[1:-1, 1:-1, 0])) and np.array_equal(_bits(X[0][:-1, :-1, -1]), _bits(one[1:-1, 1:-1, -1]))
    assert np.array_equal(_bits(X[1][:-1, 0, :-1]), _bits(one[1:-1, 0, 1:-1])) and np.array_equal(_bits(X[1][:-1, -1, :-1]), _bits(one[1:-1, -1, 1:-1]))
    assert np.array_equal(_bits(X[2][0, :-1, :-1]), _bits(one[0, 1:-1, 1:-1])) and np.array_equal(_bits(X[2][-1, :-1, :-1]), _bits(one[-1, 1:-1, 1:-1]))
    want = R.solve(n, B.DX, one, rho, FOURPI)
    phi = start.copy()
    got = B.solve(plan, phi, X, rho, FOURPI)
    assert want[1] and got[0] == want[0] and got[0] > 0
    assert np.array_equal(_bits(np.array(got[3])), _bits(np.array(want[3])))
    assert np.array_equal(_bits(phi[1:-1, 1:-1, 1:-1]), _bits(one[1:-1, 1:-1, 1:-1]))
    assert np.array_equal(_bits(phi[0]), _bits(start[0])), "the ghost zones of the level array are not written"


def test_disjoint_boxes_are_two_independent_solves():
    """layout 4: nothing couples the two boxes, and both routes have three multigrid levels with the same colours -- after the
    same number of V-cycles (the tolerances at zero: every route runs all of them, to round-off) the bits agree"""
    plan, co, cn, cbox, rho, start, X = _case("disjoint")
    assert [L.n for L in plan.lev] == [(24, 24, 24), (12, 12, 12), (6, 6, 6)]
    ncycles = 14
    phi = start.copy()
    out = B.solve(plan, phi, X, rho, FOURPI, reltol=0.0, abstol=0.0, maxiter=ncycles)
    assert out[0] == ncycles and out[2] <= 1e-10 * out[3][0]
    lo = plan.bb[0]
    for blo, bhi in plan.boxes:
        sl = tuple(slice(blo[d] - lo[d], bhi[d] - lo[d] + 1) for d in (2, 1, 0))
        gsl = tuple(slice(s.start, s.stop + 2) for s in sl)
        one = start[gsl].copy()
        A.cf_bc(one, (tuple(x - 1 for x in blo), tuple(x + 1 for x in bhi)), blo, bhi, co, cbox, cn, cbox, 0.3)
        w = R.solve((8, 8, 8), B.DX, one, rho[sl], FOURPI, reltol=0.0, abstol=0.0, maxiter=ncycles)
        assert w[0] == ncycles
        assert np.array_equal(_bits(phi[gsl][1:-1, 1:-1, 1:-1]), _bits(one[1:-1, 1:-1, 1:-1])), (blo, bhi)
    unc = ~plan.covered()
    assert np.array_equal(_bits(phi[1:-1, 1:-1, 1:-1][unc]), _bits(start[1:-1, 1:-1, 1:-1][unc])), "uncovered zones are not written"


@pytest.mark.parametrize("name", ["ell", "edge", "unequal", "wide_bottom"])
def test_masked_solve_converges_on_the_irregular_layouts(name):
    plan, co, cn, cbox, rho, start, X = _case(name)
    phi = start.copy()
    cycles, ok, norm, hist = B.solve(plan, phi, X, rho, FOURPI)
    b = np.where(plan.covered(), FOURPI * rho, 0.0)
    assert ok and 0 < cycles <= 20 and norm <= R.stopping_tolerance(b[plan.covered()])
    assert B.masked_residual64(plan, phi, X, b) == norm
    unc = ~plan.covered()
    assert np.array_equal(_bits(phi[1:-1, 1:-1, 1:-1][unc]), _bits(start[1:-1, 1:-1, 1:-1][unc]))
    g = B.grad_phi(plan, phi, X)
    assert np.isfinite(g[:, plan.covered()]).all() and np.isnan(g[:, unc]).all()


# ---- 2. the driver on the CPU backend --------------------------------------------------------------------------------------------
def test_several_boxes_are_accepted_and_solved(oracle):
    a = _amr(oracle, patches=[ELL_CRSE])
    a.initData("dust_collapse", **R.DUST_PROB)
    assert len(a.lev) == 2 and len(a.lev[1].boxes) == 3
    dt = a.step()
    g = a.gravity
    ent = g._lev[1]
    assert dt > 0.0 and ent["boxes"] == tuple(B.LAYOUTS["ell"]) and isinstance(ent["plan"], B.Plan)
    assert ent["phibox"] == ((7, 7, 7), (24, 24, 16)) and ent["faces"].shape == (3, 9, 17, 17)
    with pytest.raises(ValueError, match="phi_grav_level"):
        a.phi_grav(1)
    box, phi, cov = a.phi_grav_level(1)
    assert box == ((8, 8, 8), (23, 23, 15)) and phi.shape == cov.shape == (8, 16, 16) and int(cov.sum()) == 3 * 512
    assert np.isfinite(phi[cov]).all() and np.all(phi[cov] < 0.0) and np.all(phi[~cov] == 0.0), "uncovered zones are never written"
    box0, phi0, cov0 = a.phi_grav_level(0)
    assert box0 == ((0, 0, 0), (15, 15, 15)) and cov0.all()
    assert np.array_equal(_bits(phi0), _bits(a.phi_grav(0).numpy()[0, 1:-1, 1:-1, 1:-1]))
    st = a.poisson_stats(1)
    assert st["first"]["cycles"] > 0 and st["new"]["norm"] <= 1e-10 * st["new"]["history"][0]
    assert [s[0] for s in g.solve_log].count(1) >= 4
    for b in a.lev[1].boxes:
        assert np.isfinite(b.grav_new.numpy()).all() and np.isfinite(b.S_new().numpy()).all()
    a.close()
    assert all(e["plan"] is None for e in g._lev.values())


def test_a_second_level_of_two_boxes_nested_in_the_ell(oracle):
    a = _amr(oracle, patches=[ELL_CRSE, NESTED2], max_level=2)
    a.initData("dust_collapse", **R.DUST_PROB)
    assert [len(l.boxes) for l in a.lev] == [1, 3, 2]
    a.step()
    box, phi, cov = a.phi_grav_level(2)
    assert int(cov.sum()) == 2 * 512 and np.isfinite(phi[cov]).all()
    a.close()


def test_the_nesting_rule_names_the_box(oracle):
    """a level-2 box whose coarsened box, grown by one, reaches into the notch of the ell: level-1 zones 15..20 in x and y"""
    bad = [((10, 10, 10), (13, 13, 13)), ((16, 16, 10), (19, 19, 13))]
    with pytest.raises(ValueError, match=r"the box \(\(32, 32, 20\), \(39, 39, 27\)\) of level 2.*does not lie inside the union"):
        _amr(oracle, patches=[ELL_CRSE, bad], max_level=2)


def test_the_bottom_limit_names_the_level_and_the_bounding_box(oracle):
    """two boxes aligned to 2 zones at the ends of a bounding box of 36^3 zones: the level coarsens once, to 18^3 = 5832 zones,
    more than CASTRO_AMD_POISSON_MAX_BOTTOM = 4096"""
    import castro_amd
    g = castro_amd.PoissonGravity()
    boxes = [((2, 2, 2), (5, 5, 5)), ((34, 34, 34), (37, 37, 37))]
    with pytest.raises(ValueError, match=r"level 1 with the bounding box \(\(2, 2, 2\), \(37, 37, 37\)\).*aligned to 2 zones.*"
                                         r"CASTRO_AMD_POISSON_MAX_BOTTOM"):
        g._check_bottom_boxes(1, boxes)
    with pytest.raises(ValueError, match="MAX_BOTTOM|more than"):
        B.Plan(B.DX, boxes)
    g._check_bottom_boxes(1, B.LAYOUTS["unequal"])


def test_the_old_backend_keeps_the_refusal(oracle):
    with pytest.raises(NotImplementedError, match="level 1 would have 3 boxes.*poisson_boxes_plan_create"):
        _amr(oracle, patches=[ELL_CRSE], make_hydro=lambda: A.PoissonAmrOracleBackend())


def _clustered(oracle):
    """the tagged, clustered level 1 of tests/poisson_boxes_ref.py"""
    a = _amr(oracle, **B.CLUSTER_KW)
    a.initData("dust_collapse", **B.CLUSTER_PROB)
    return a


def test_a_regrid_that_changes_the_box_list_remakes_the_arrays_and_the_plan(oracle):
    a = _clustered(oracle)
    assert len(a.lev) == 2 and len(a.lev[1].boxes) > 1, "the tag threshold must give a level of several boxes"
    a.step()
    g = a.gravity
    key0, plan0 = g._lev[1]["key"], g._lev[1]["plan"]
    assert key0 == tuple(b.bx for b in a.lev[1].boxes) and plan0 is not None
    assert a.poisson_stats(1)["new"]["norm"] <= 1e-10 * a.poisson_stats(1)["new"]["history"][0]
    a.n_error_buf = 1
    assert a.regrid(0)
    assert 1 not in g._lev, "the potential and the plan of the level that was re-made are gone"
    a.step()
    assert g._lev[1]["key"] == tuple(b.bx for b in a.lev[1].boxes) != key0 and g._lev[1]["plan"] is not plan0
    box, phi, cov = a.phi_grav_level(1)
    assert np.isfinite(phi[cov]).all()
    a.close()

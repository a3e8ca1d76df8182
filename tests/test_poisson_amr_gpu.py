"""GPU tests of Poisson gravity on the levels of CastroAmr, for both numerics builds: k_phi_cf_bc against the restatement
(tests/poisson_amr_ref.py) bit for bit in both builds, the solve of a patch through the single-level entry points, and the two
driver runs of tests/test_poisson_amr_cpu.py on the device against the run on PoissonAmrOracleBackend."""
import numpy as np
import pytest
import torch

from tests import monopole_ref as MR
from tests import poisson_amr_ref as A
from tests import poisson_ref as R

pytestmark = pytest.mark.gpu

_CACHE = {}
PATCHES = {"cube": ((4, 4, 4), (11, 11, 11)), "slab": ((2, 4, 6), (5, 11, 13))}       # coarse zones of a 16^3 level
SENT = -4.25e33


@pytest.fixture(scope="module", params=["exact", "contract"])
def hydro(request):
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=request.param)
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shape(box):
    return tuple(box[1][d] - box[0][d] + 1 for d in (2, 1, 0))


def _coarse():
    """random coarse potentials of a 16^3 level: the old one on the level grown by one, the new one on the level grown by two"""
    if "coarse" not in _CACHE:
        rng = np.random.default_rng(41)
        ob, nb = ((-1, -1, -1), (16, 16, 16)), ((-2, -2, -2), (17, 17, 17))
        _CACHE["coarse"] = (rng.normal(size=_shape(ob)) * 3.0 - 7.0, ob, rng.normal(size=_shape(nb)) * 3.0 - 7.0, nb)
    return _CACHE["coarse"]


def _fine(patch):
    flo, fhi = tuple(2 * x for x in patch[0]), tuple(2 * x + 1 for x in patch[1])
    return flo, fhi, (tuple(x - 3 for x in flo), tuple(x + 3 for x in fhi))     # the FAB: the patch grown by three


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [0.0, 0.3, 0.5, 1.0])
@pytest.mark.parametrize("patch", sorted(PATCHES))
def test_cf_bc_kernel_against_the_restatement(hydro, patch, a):
    """no contraction in either build: the same bits as the restatement in `exact` and in `contract`; only the one-zone shell of
    the patch is written"""
    co, ob, cn, nb = _coarse()
    flo, fhi, fbox = _fine(PATCHES[patch])
    want = np.full(_shape(fbox), SENT)
    A.cf_bc(want, fbox, flo, fhi, co, ob, cn, nb, a)
    phi = torch.full((1,) + want.shape, SENT, dtype=torch.float64, device="cuda")
    hydro.poisson_cf_bc(phi, fbox, flo, fhi, _dev(co[None]), ob, _dev(cn[None]), nb, a)
    torch.cuda.synchronize()
    got = phi.cpu().numpy()[0]
    shell = np.zeros(want.shape, dtype=bool)
    shell[2:-2, 2:-2, 2:-2] = True
    shell[3:-3, 3:-3, 3:-3] = False
    assert np.all(want[~shell] == SENT) and np.all(want[shell] != SENT)
    assert np.array_equal(_bits(got[~shell]), _bits(want[~shell])), "valid zones and everything outside the shell keep the sentinel"
    d = _bits(got[shell]) != _bits(want[shell])
    assert not d.any(), "%d of %d shell zones differ, max %g" % (int(d.sum()), d.size, np.abs(got - want)[shell].max())
    assert np.all(got[2, 2, 2:-2] == 0.0) and np.all(got[2, 2:-2, 2] == 0.0) and got[-3, -3, -3] == 0.0, "edges and corners"


def test_cf_bc_refuses_bad_coverage(hydro):
    co, ob, cn, nb = _coarse()
    O, N = _dev(co[None]), _dev(cn[None])
    flo, fhi, fbox = _fine(PATCHES["cube"])
    phi = torch.zeros((1,) + _shape(fbox), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="bad argument"):                 # the fine FAB does not hold the shell of this box
        hydro.poisson_cf_bc(phi, fbox, (0, 8, 8), (7, 23, 23), O, ob, N, nb, 0.5)
    small = ((0, 0, 0), (15, 15, 15))                                       # a coarse FAB without the zones around the domain
    flo2, fhi2 = (0, 8, 8), (7, 23, 23)
    fb2 = (tuple(x - 1 for x in flo2), tuple(x + 1 for x in fhi2))
    phi2 = torch.zeros((1,) + _shape(fb2), dtype=torch.float64, device="cuda")
    Os = _dev(co[None, 1:-1, 1:-1, 1:-1])
    with pytest.raises(RuntimeError, match="bad argument"):                 # coarse zone -1 is read and the old FAB does not hold it
        hydro.poisson_cf_bc(phi2, fb2, flo2, fhi2, Os, small, N, nb, 0.5)
    with pytest.raises(RuntimeError, match="bad argument"):                 # ... nor the new one
        hydro.poisson_cf_bc(phi2, fb2, flo2, fhi2, O, ob, Os, small, 0.5)
    with pytest.raises(RuntimeError, match="bad argument"):                 # an odd low corner is not the refinement of a coarse box
        hydro.poisson_cf_bc(phi, fbox, (9, 8, 8), fhi, O, ob, N, nb, 0.5)
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.poisson_cf_bc(phi, fbox, flo, (22, 23, 23), O, ob, N, nb, 0.5)
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.poisson_cf_bc(phi, fbox, flo, fhi, O, ob, N, nb, float("nan"))
    three = torch.zeros((3,) + _shape(fbox), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.poisson_cf_bc(three, fbox, flo, fhi, O, ob, N, nb, 0.5)
    hydro.poisson_cf_bc(phi2, fb2, flo2, fhi2, O, ob, N, nb, 0.5)            # the same box with FABs that hold what is read
    torch.cuda.synchronize()
    assert np.isfinite(phi2.cpu().numpy()).all()


# ---- 2. the solve of a patch through the single-level entry points ---------------------------------------------------------------
def _patch_case(patch):
    """density and starting potential of the fine zones of a patch of a 32^3 level of the unit cube, the boundary values from the
    random coarse potentials at a = 0.3; the restatement's solve"""
    key = ("solve", patch)
    if key not in _CACHE:
        co, ob, cn, nb = _coarse()
        flo, fhi, _ = _fine(PATCHES[patch])
        n = tuple(fhi[d] - flo[d] + 1 for d in range(3))
        rng = np.random.default_rng(5)
        rho = rng.uniform(0.5, 2.0, size=n[::-1])
        pbox = (tuple(x - 1 for x in flo), tuple(x + 1 for x in fhi))
        start = np.zeros(_shape(pbox))
        start[1:-1, 1:-1, 1:-1] = rng.normal(size=n[::-1]) - 7.0
        A.cf_bc(start, pbox, flo, fhi, co, ob, cn, nb, 0.3)
        phi = start.copy()
        out = R.solve(n, (1.0 / 32,) * 3, phi, rho, 4.0 * np.pi)
        _CACHE[key] = (rho, start, phi, out, flo, fhi, pbox, n)
    return _CACHE[key]


@pytest.mark.parametrize("patch", sorted(PATCHES))
def test_patch_solve_through_the_single_level_entry_points(hydro, patch):
    """a geometry whose domain is the patch, a density FAB that contains the patch rather than equals it: `exact` gives the
    restatement's cycle count, norm history and phi bit for bit; `contract` meets the stopping rule on a residual recomputed in
    float64 and, on the smaller patch, the dense bound -- the allowances of tests/test_poisson_gpu.py::test_poisson_solve"""
    from castro_amd import _lib
    rho, start, wphi, (wcycles, wok, wnorm, whist), flo, fhi, pbox, n = _patch_case(patch)
    assert wok
    geom = _lib.make_geom((32, 32, 32))
    dx = tuple(geom.dx[d] for d in range(3))
    assert dx == (1.0 / 32,) * 3
    for d in range(3):
        geom.domlo[d], geom.domhi[d] = flo[d], fhi[d]
    ubox = ((-2, -2, -2), (33, 33, 33))                                     # the density: component 1 of a FAB of the whole level
    U = np.full((3,) + _shape(ubox), np.nan)
    U[(1,) + tuple(slice(flo[d] + 2, fhi[d] + 3) for d in (2, 1, 0))] = rho
    Ud = _dev(U)
    plan = hydro.poisson_plan_create(geom)
    try:
        P = _dev(start[None])
        cycles, ok, norm, hist = hydro.poisson_solve(plan, P, pbox, Ud, ubox, 1, 4.0 * np.pi)
        torch.cuda.synchronize()
        got = P.cpu().numpy()[0]
        shell = np.ones(got.shape, dtype=bool)
        shell[1:-1, 1:-1, 1:-1] = False
        assert np.array_equal(_bits(got[shell]), _bits(start[shell])), "the boundary values are not written"
        b = 4.0 * np.pi * rho
        tol = R.stopping_tolerance(b)
        print("patch %s (%s): %d cycles (restatement %d), final norm %.3g, tolerance %.3g" % (patch, hydro.numerics, cycles, wcycles, norm, tol))
        assert ok and norm <= tol and len(hist) == cycles + 3
        if hydro.numerics == "exact":
            assert cycles == wcycles
            assert np.array_equal(_bits(np.array(hist)), _bits(np.array(whist))), (hist, whist)
            assert np.array_equal(_bits(got), _bits(wphi))
        else:
            L0 = R.levels(n, dx)[0]
            rr = np.abs(R.residual(L0, got, b)).max()
            assert rr <= tol, (rr, tol)
            if patch == "slab":
                dev, bound = R.dense_check(L0, got, b)
                print("dense check (contract): deviation %.3g, bound %.3g" % (dev, bound))
                assert dev <= bound
        # g = -grad(phi) of the patch through the same geometry
        gbox = pbox
        G = torch.full((3,) + _shape(gbox), float("nan"), dtype=torch.float64, device="cuda")
        hydro.grad_phi_to_grav(P, pbox, G, gbox, geom)
        torch.cuda.synchronize()
        gg = G.cpu().numpy()
        mag = np.zeros((3,) + n[::-1])
        wg = R.grad_phi(got, dx, mag)
        assert np.isnan(gg[:, 0]).all() and np.isnan(gg[:, :, :, -1]).all()
        if hydro.numerics == "exact":
            assert np.array_equal(_bits(gg[:, 1:-1, 1:-1, 1:-1]), _bits(wg))
        else:
            assert np.all(np.abs(gg[:, 1:-1, 1:-1, 1:-1] - wg) <= 8.0 * R.U52 * mag)
    finally:
        hydro.poisson_plan_destroy(plan)


# ---- 3. the driver ---------------------------------------------------------------------------------------------------------------
def _reference(oracle, case):
    if ("ref", case) not in _CACHE:
        ref, dts, s = A.dust_amr_sensitivity(oracle, case)
        _CACHE[("ref", case)] = (A.level_fields(ref), dts, s, list(ref.gravity.solve_log),
                                 [ref.poisson_stats(l) for l in range(len(ref.lev))])
    return _CACHE[("ref", case)]


def test_boundary_potential_at_order_zero_is_the_restatement_bit_for_bit(hydro):
    """with lnum = 0 the boundary potential holds no library call (r^(-1) is one division): the bits of poisson_amr_ref.phi_bc in
    both builds, on a cubic domain with the centre in the middle and on a non-cubic one with the centre off it"""
    from castro_amd import _lib
    for n, hi, center, q0 in (((16, 16, 16), (1.5e9, 1.5e9, 1.5e9), (7.5e8, 7.5e8, 7.5e8), 5.24703829e+08),
                              ((12, 8, 10), (1.5, 1.0, 1.25), (0.4, 0.7, 0.3), 1.2345678)):
        geom = _lib.make_geom(n, prob_hi=hi)
        mp = _lib.make_multipole(geom, center, 0)
        q = np.array([q0, 0.0, 0.0])
        box = ((-1, -1, -1), n)
        want = np.full((n[2] + 2, n[1] + 2, n[0] + 2), SENT)
        A.phi_bc(q, geom, mp, want, box)
        phi = torch.full((1,) + want.shape, SENT, dtype=torch.float64, device="cuda")
        hydro.multipole_phi_bc(phi, box, geom, mp, _dev(q))
        torch.cuda.synchronize()
        got = phi.cpu().numpy()[0]
        assert np.all(want[1:-1, 1:-1, 1:-1] == SENT) and (want != SENT).sum() == want.size - n[0] * n[1] * n[2]
        d = _bits(got) != _bits(want)
        assert not d.any(), "%s: %d zones differ" % (n, int(d.sum()))


@pytest.mark.parametrize("case", ["one", "two"])
def test_dust_collapse_amr_driver_against_the_cpu_backend(hydro, oracle, case):
    """The dust collapse on 16^3 + one 16^3 patch, and + a second nested one, two coarse steps, against the same driver on
    PoissonAmrOracleBackend (moments summed in the device's order).  `exact`: S_new, phi and g of every level bit for bit.
    `contract`: per field and level within max(1e-10, 100 s) of the field's max, s the deviation the CPU backend shows between
    two runs whose moments differ by a factor 1 + 2^-52 (the rule of the single-level test); phi and g within 1e-8 of their max."""
    import castro_amd
    from castro_amd import _lib
    want, dts, s, wlog, wst = _reference(oracle, case)
    a, gdts = A.dust_amr_run(lambda: castro_amd.HipHydro(0, numerics=hydro.numerics), _lib.default_params(**R.DUST_PARAMS), case)
    torch.cuda.synchronize()
    got = A.level_fields(a)
    assert a.gravity.solve_log == wlog
    for l, ((wS, wphi, wg), (gS, gphi, gg)) in enumerate(zip(want, got)):
        dS = MR.field_deviation(gS, wS)
        dphi = np.abs(gphi - wphi).max() / np.abs(wphi).max()
        dg = np.abs(gg - wg).max() / np.abs(wg).max()
        st = a.poisson_stats(l)
        print("AMR dust collapse %s (%s) level %d: state deviation" % (case, hydro.numerics, l), dS, "s", s[l],
              "phi %.3g g %.3g, cycles first / new %d / %d (CPU backend %d / %d)"
              % (dphi, dg, st["first"]["cycles"], st["new"]["cycles"], wst[l]["first"]["cycles"], wst[l]["new"]["cycles"]))
    print("dts", gdts, dts)
    for l, ((wS, wphi, wg), (gS, gphi, gg)) in enumerate(zip(want, got)):
        if hydro.numerics == "exact":
            assert np.array_equal(_bits(gS), _bits(wS)), "S_new of level %d" % l
            assert np.array_equal(_bits(gphi), _bits(wphi)), "phi of level %d" % l
            assert np.array_equal(_bits(gg), _bits(wg)), "g of level %d" % l
        else:
            tol = np.maximum(1e-10, 100.0 * s[l])
            assert np.all(MR.field_deviation(gS, wS) <= tol), (l, MR.field_deviation(gS, wS), tol)
            assert np.abs(gphi - wphi).max() <= 1e-8 * np.abs(wphi).max()
            assert np.abs(gg - wg).max() <= 1e-8 * np.abs(wg).max()
    if hydro.numerics == "exact":
        assert gdts == dts
    else:
        assert np.allclose(np.array(gdts), np.array(dts), rtol=1e-12, atol=0.0), (gdts, dts)
    a.close()
    assert all(ent["plan"] is None for ent in a.gravity._lev.values())


def test_single_level_and_level_zero_are_one_route(hydro):
    """Castro(poisson=...) and a CastroAmr(gravity=...) with no refined level, two whole steps from the same state on the device:
    the same launches on buffers of the same extents, so the same bits in either build"""
    import castro_amd
    from castro_amd import _lib
    c, a = A.single_and_hierarchy(lambda: castro_amd.HipHydro(0, numerics=hydro.numerics), _lib.default_params(**R.DUST_PARAMS))
    torch.cuda.synchronize()
    A.assert_routes_agree(c, a)
    c.close()
    a.close()

"""GPU tests of Poisson gravity (castro_amd/csrc/poisson_kernels.hip and Castro(poisson=PoissonGravity(...))), for both numerics
builds.  Reference and tolerances: tests/poisson_ref.py -- the moments and the boundary potential within the summation-order
bound plus the per-call allowance derived there, the multigrid passes, the solve and the gradient bit for bit in the `exact`
build and within 8 * 2^-52 of the term magnitudes (passes) or under the stopping rule and the dense bound (solve) in `contract`,
the driver within max(1e-10, 100 s) of the field's max."""
import numpy as np
import pytest
import torch

from tests import grid_caps as G
from tests import monopole_ref as MR
from tests import poisson_ref as R
from tests.test_monopole_gpu import N_CELL, PROB_HI, _bin_boxes

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
# the last two: bottom solves of 2176 and 1470 x-pairs per colour, three and two trips of the one workgroup (tests/grid_caps.py)
SHAPES = [(16, 16, 16), (16, 8, 12), (6, 10, 14), (5, 7, 9)] + G.BOTTOM_ONE_BOX
DX = (0.11, 0.13, 0.09)
FOURPIG = 4.0 * np.pi * 6.67428e-8
_CACHE = {}


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


# ---- moments ---------------------------------------------------------------------------------------------------------------------
CENTERS = {"mid": (1.5, 1.25, 1.0), "off": (0.9, 1.7, 0.55)}


@pytest.mark.parametrize("lnum", [0, 2, 6, G.MP_ORDER])           # the last: CASTRO_AMD_MAX_MULTIPOLE, every column of a row in use
@pytest.mark.parametrize("where", ["mid", "off"])
def test_multipole_moments(hydro, lnum, where):
    from castro_amd import _lib
    geom = _lib.make_geom(N_CELL, prob_hi=PROB_HI)
    mp = _lib.make_multipole(geom, CENTERS[where], lnum)
    boxes = _bin_boxes()
    key = ("mom", lnum, where)
    if key not in _CACHE:
        _CACHE[key] = R.moments([(rho, lo, mask) for rho, lo, hi, mask, F, fbox in boxes], geom, mp)
    want, bound = _CACHE[key]
    dev = [(_dev(F), None if mask is None else _dev(mask)) for _, _, _, mask, F, _ in boxes]
    table = hydro.make_diag_boxes([(b[1], b[2], (d[0], b[5]), d[1]) for b, d in zip(boxes, dev)])
    n = 3 * (lnum + 1) ** 2

    def call(stream=None):
        out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        hydro.multipole_moments_mf(table, geom, mp, out, stream=stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    got = call()
    err = np.abs(got - want)
    live = bound > 0
    worst = float((err[live] / bound[live]).max())
    print("moments lnum %d centre %s (%s): worst deviation / bound = %.3g over %d moments" % (lnum, where, hydro.numerics, worst,
                                                                                             int(live.sum())))
    assert live.sum() == (lnum + 1) + lnum * (lnum + 1)          # qL0(l), and qLC / qLS for 1 <= m <= l
    assert np.all(got[~live] == 0.0), "entries the loop nest does not reach are zero"
    assert np.all(err <= bound), (err[live] / bound[live])
    again = call()
    assert np.array_equal(_bits(again), _bits(got)), "two calls: the same bits"
    other = call(stream=torch.cuda.Stream())
    assert np.array_equal(_bits(other), _bits(got)), "another stream: the same bits"


def test_multipole_refuses_an_order_above_the_cap(hydro):
    from castro_amd import _lib
    geom = _lib.make_geom(N_CELL, prob_hi=PROB_HI)
    mp = _lib.make_multipole(geom, CENTERS["mid"], 2)
    mp.lnum = _lib.MAX_MULTIPOLE + 1
    b = _bin_boxes()[0]
    table = hydro.make_diag_boxes([(b[1], b[2], (_dev(b[4]), b[5]), None)])
    out = torch.zeros(3 * (mp.lnum + 1) ** 2, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        hydro.multipole_moments_mf(table, geom, mp, out)


# ---- boundary potential ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lnum,where", [(0, "mid"), (6, "off"), (2, "corner"), (G.MP_ORDER, "off")])
def test_multipole_phi_bc(hydro, lnum, where):
    """the ghost shell against the restatement from the same moments; valid zones keep their sentinel bits; with the centre on the
    high corner of the domain the corner ghost zone has r = 0 and phi exactly 0"""
    from castro_amd import _lib
    n = (12, 8, 10)
    geom = _lib.make_geom(n, prob_hi=(1.5, 1.0, 1.25))          # zones of 0.125
    center = {"mid": (0.75, 0.5, 0.625), "off": (0.4, 0.7, 0.3), "corner": (1.5, 1.0, 1.25)}[where]
    mp = _lib.make_multipole(geom, center, lnum)
    rng = np.random.default_rng(31 + lnum)
    q, _ = R.moments([(rng.uniform(1.0e5, 2.0e5, size=(n[2], n[1], n[0])), (0, 0, 0), None)], geom, mp)
    box = ((-1, -1, -1), n)
    SENT = -4.25e33
    want = np.full((n[2] + 2, n[1] + 2, n[0] + 2), SENT)
    outside, allow = R.phi_bc(q, geom, mp, want, box)
    phi = torch.full((1,) + want.shape, SENT, dtype=torch.float64, device="cuda")
    hydro.multipole_phi_bc(phi, box, geom, mp, _dev(q))
    torch.cuda.synchronize()
    got = phi.cpu().numpy()[0]
    assert np.array_equal(_bits(got[~outside]), _bits(want[~outside])), "valid zones are not written"
    err = np.abs(got - want)[outside]
    a = allow[outside]
    live = a > 0
    print("phi_bc lnum %d centre %s (%s): worst deviation / allowance = %.3g" % (lnum, where, hydro.numerics,
                                                                             float((err[live] / a[live]).max())))
    assert np.all(err <= a)
    assert np.all(got[outside] != SENT)
    if where == "corner":
        assert got[-1, -1, -1] == 0.0 and want[-1, -1, -1] == 0.0


# ---- level operations ------------------------------------------------------------------------------------------------------------
def _grown(valid, ng, ghost=None):
    """`valid` (nz, ny, nx) inside a FAB grown by ng zones of NaN; ghost: a one-ghost array whose shell goes around the valid zones"""
    F = np.full(tuple(s + 2 * ng for s in valid.shape), np.nan)
    if ghost is not None:
        s = ng - 1
        F[s:F.shape[0] - s, s:F.shape[1] - s, s:F.shape[2] - s] = ghost
    F[ng:-ng, ng:-ng, ng:-ng] = valid
    return F


def _box(L, ng):
    return (tuple([-ng] * 3), tuple(v - 1 + ng for v in L.n))


def _check(h, got, want, mag, what):
    """`exact`: the same bits; `contract`: within 8 * 2^-52 of the sum of the magnitudes of the terms of each result"""
    if h.numerics == "exact":
        assert np.array_equal(got, want), "%s: %d entries differ, max %g" % (what, int((got != want).sum()), np.nanmax(np.abs(got - want)))
    else:
        d = np.abs(got - want)
        print("%s (contract): worst deviation / (8 * 2^-52 * magnitude) = %.3g" % (what, float((d / (8.0 * U52 * mag + 1e-300)).max())))
        assert np.all(d <= 8.0 * U52 * mag), what


def test_level_operations(hydro):
    """every pass on (16, 8, 12) with zones of three widths, on FABs that hold NaN beyond the zones a pass may read"""
    from castro_amd import _lib
    n = (16, 8, 12)
    geom = _lib.make_geom(n, prob_hi=tuple(n[d] * DX[d] for d in range(3)))
    assert all(geom.dx[d] == (n[d] * DX[d]) / n[d] for d in range(3))
    dx = tuple(geom.dx[d] for d in range(3))
    lev = R.levels(n, dx)
    plan = hydro.poisson_plan_create(geom)
    rng = np.random.default_rng(8)
    try:
        for l in (0, 1, 2):
            L = lev[l]
            p1 = rng.normal(size=L.gshape)                       # a one-ghost phi, ghost values included
            b = rng.normal(size=L.shape) * 10.0
            P = _dev(_grown(p1[1:-1, 1:-1, 1:-1], 3, p1)[None])
            B = _dev(_grown(b, 2)[None])
            # smoother, colour 0 then colour 1 on top of it
            want = p1.copy()
            for colour in (0, 1):
                mag = np.zeros(L.shape)
                prev = want.copy()
                R.smooth(L, want, b, colour, mag)
                hydro.poisson_level_op(plan, _lib.MG_SMOOTH, l, (P, _box(L, 3)), (B, _box(L, 2)), colour=colour)
                torch.cuda.synchronize()
                got = P.cpu().numpy()[0]
                assert np.isnan(got[0]).all() and np.isnan(got[:, :, 1]).all(), "nothing beyond the ghost zone is touched"
                g1 = got[2:-2, 2:-2, 2:-2]
                assert np.array_equal(_bits(g1[0]), _bits(p1[0])) and np.array_equal(_bits(g1[:, :, -1]), _bits(p1[:, :, -1]))
                sel = R._faces(L)[1] == colour
                assert np.array_equal(_bits(g1[1:-1, 1:-1, 1:-1][~sel]), _bits(prev[1:-1, 1:-1, 1:-1][~sel])), "the other colour stays"
                _check(hydro, g1[1:-1, 1:-1, 1:-1][sel], want[1:-1, 1:-1, 1:-1][sel], mag[sel], "smoother level %d colour %d" % (l, colour))
                if hydro.numerics != "exact":
                    want = g1.copy()                             # the next sweep starts from what the device holds
            # residual
            mag = np.zeros(L.shape)
            wres = R.residual(L, want, b, mag)
            RS = _dev(_grown(np.zeros(L.shape), 1)[None])
            hydro.poisson_level_op(plan, _lib.MG_RESIDUAL, l, (P, _box(L, 3)), (B, _box(L, 2)), (RS, _box(L, 1)))
            torch.cuda.synchronize()
            gres = RS.cpu().numpy()[0]
            assert np.isnan(gres[0]).all()
            _check(hydro, gres[1:-1, 1:-1, 1:-1], wres, mag, "residual level %d" % l)
            # norm
            out = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
            hydro.poisson_level_op(plan, _lib.MG_NORM, l, (RS, _box(L, 1)), out=out)
            torch.cuda.synchronize()
            held = gres[1:-1, 1:-1, 1:-1]
            assert tuple(out.cpu().numpy()) == (np.abs(held).max(), held.max())
            if l + 1 < len(lev):
                C = lev[l + 1]
                # restriction of the residual the device holds
                mag = np.zeros(C.shape)
                wb = R.restrict(held, mag)
                BC = _dev(_grown(np.full(C.shape, 7.0), 2)[None])
                PC = _dev(_grown(np.full(C.shape, 7.0), 1, np.full(C.gshape, 5.0))[None])
                hydro.poisson_level_op(plan, _lib.MG_RESTRICT, l, (RS, _box(L, 1)), (BC, _box(C, 2)), (PC, _box(C, 1)))
                torch.cuda.synchronize()
                _check(hydro, BC.cpu().numpy()[0][2:-2, 2:-2, 2:-2], wb, mag, "restriction level %d" % l)
                pc = PC.cpu().numpy()[0]
                assert np.all(pc[1:-1, 1:-1, 1:-1] == 0.0) and np.all(pc[0] == 5.0) and np.all(pc[:, :, -1] == 5.0)
                # prolongation
                corr = rng.normal(size=C.shape)
                PC2 = _dev(_grown(corr, 1, np.full(C.gshape, np.nan))[None])
                before = P.cpu().numpy()[0][2:-2, 2:-2, 2:-2].copy()
                wp = before.copy()
                cg = np.zeros(C.gshape)
                cg[1:-1, 1:-1, 1:-1] = corr
                R.prolong(cg, wp)
                hydro.poisson_level_op(plan, _lib.MG_PROLONG, l, (PC2, _box(C, 1)), (P, _box(L, 3)))
                torch.cuda.synchronize()
                gp = P.cpu().numpy()[0][2:-2, 2:-2, 2:-2]
                assert np.array_equal(_bits(gp), _bits(wp)), "one addition per zone: the same bits in both builds"
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.poisson_level_op(plan, _lib.MG_RESTRICT, len(lev) - 1, (RS, _box(L, 1)), (RS, _box(L, 1)), (RS, _box(L, 1)))
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.poisson_level_op(plan, _lib.MG_SMOOTH, 0, (RS, _box(L, 1)), (B, _box(L, 2)))      # too small for level 0
    finally:
        hydro.poisson_plan_destroy(plan)


# ---- solve -----------------------------------------------------------------------------------------------------------------------
def _solve_case(n):
    from tests.test_poisson_cpu import _mg_case
    key = ("solve", n)
    if key not in _CACHE:
        rho, phi = _mg_case(n)
        start = phi.copy()
        out = R.solve(n, DX, phi, rho, FOURPIG)
        _CACHE[key] = (rho, start, phi, out)
    return _CACHE[key]


@pytest.mark.parametrize("n", SHAPES)
def test_poisson_solve(hydro, n):
    from castro_amd import _lib
    from tests.test_poisson_cpu import independent_residual
    geom = _lib.make_geom(n, prob_hi=tuple(n[d] * DX[d] for d in range(3)))
    dx = tuple(geom.dx[d] for d in range(3))
    rho, start, wphi, (wcycles, wok, wnorm, whist) = _solve_case(n)
    if dx != DX:                                                 # the restatement must see the dx the library sees
        p = start.copy()
        wcycles, wok, wnorm, whist = R.solve(n, dx, p, rho, FOURPIG)
        wphi = p
    U = np.full((3, n[2] + 4, n[1] + 4, n[0] + 4), np.nan)        # the density is component 1 of a FAB with two NaN ghost zones
    U[1, 2:-2, 2:-2, 2:-2] = rho
    Ud = _dev(U)
    ubox = ((-2, -2, -2), tuple(v + 1 for v in n))
    pbox = ((-1, -1, -1), n)
    plan = hydro.poisson_plan_create(geom)
    try:
        def run():
            P = _dev(start[None])
            out = hydro.poisson_solve(plan, P, pbox, Ud, ubox, 1, FOURPIG)
            torch.cuda.synchronize()
            return P.cpu().numpy()[0], out
        got, (cycles, ok, norm, hist) = run()
        again, out2 = run()
        assert np.array_equal(_bits(again), _bits(got)) and out2[3] == hist, "two solves from the same start: the same bits"
        shell = np.ones(got.shape, dtype=bool)
        shell[1:-1, 1:-1, 1:-1] = False
        assert np.array_equal(_bits(got[shell]), _bits(start[shell])), "the boundary values are not written"
        b = FOURPIG * rho
        tol = R.stopping_tolerance(b)
        print("solve %s (%s): %d cycles (restatement %d), final norm %.3g, tolerance %.3g" % (n, hydro.numerics, cycles, wcycles, norm, tol))
        assert ok and norm <= tol and len(hist) == cycles + 3
        if hydro.numerics == "exact":
            assert cycles == wcycles
            assert np.array_equal(_bits(np.array(hist)), _bits(np.array(whist))), (hist, whist)
            assert np.array_equal(_bits(got), _bits(wphi))
        else:
            L = R.levels(n, dx)[0]
            rr = np.abs(R.residual(L, got, b)).max()
            assert rr <= tol, (rr, tol)
            if n == (16, 8, 12):
                dev, bound = R.dense_check(L, got, b)
                print("dense check (contract): deviation %.3g, bound %.3g" % (dev, bound))
                assert dev <= bound
    finally:
        hydro.poisson_plan_destroy(plan)


def test_plan_creation_is_refused_for_an_extent_with_too_few_factors_of_two(hydro):
    from castro_amd import _lib
    with pytest.raises(ValueError, match=r"n_cell = \(250, 250, 250\)"):
        hydro.poisson_plan_create(_lib.make_geom((250, 250, 250)))
    with pytest.raises(ValueError, match="periodic or Symmetry"):
        hydro.poisson_plan_create(_lib.make_geom((16, 16, 16), lo_bc=(3, 2, 2)))


# ---- gravity from phi ------------------------------------------------------------------------------------------------------------
def test_grad_phi_to_grav(hydro):
    from castro_amd import _lib
    n = (16, 8, 12)
    geom = _lib.make_geom(n, prob_hi=tuple(n[d] * DX[d] for d in range(3)), lo_bc=(2, 1, 4), hi_bc=(2, 5, 2))
    dx = tuple(geom.dx[d] for d in range(3))
    rng = np.random.default_rng(77)
    p1 = rng.normal(size=(n[2] + 2, n[1] + 2, n[0] + 2))
    P = _dev(_grown(p1[1:-1, 1:-1, 1:-1], 2, p1)[None])
    gbox = ((-1, -1, -1), n)
    G = torch.full((3, n[2] + 2, n[1] + 2, n[0] + 2), float("nan"), dtype=torch.float64, device="cuda")
    hydro.grad_phi_to_grav(P, ((-2, -2, -2), tuple(v + 1 for v in n)), G, gbox, geom)
    torch.cuda.synchronize()
    got = G.cpu().numpy()
    mag = np.zeros((3, n[2], n[1], n[0]))
    want = R.grad_phi(p1, dx, mag)
    assert np.isnan(got[:, 0]).all() and np.isnan(got[:, :, :, -1]).all(), "the ghost zone is left to the boundary fill"
    _check(hydro, got[:, 1:-1, 1:-1, 1:-1], want, mag, "gravity from phi")
    hydro.grav_bc_fill(G, gbox, geom)
    torch.cuda.synchronize()
    full = np.full(got.shape, np.nan)
    full[:, 1:-1, 1:-1, 1:-1] = got[:, 1:-1, 1:-1, 1:-1]
    R.grav_bc_fill(full, gbox, geom)
    assert np.array_equal(_bits(G.cpu().numpy()), _bits(full)), "the ghost zone is the Gravity_Type fill of the valid zones"


# ---- driver ----------------------------------------------------------------------------------------------------------------------
def test_dust_collapse_driver_against_the_restatement(hydro, oracle):
    """Dust collapse, 16^3, the full star, 3 steps, against the same driver on PoissonOracleBackend.  Not bitwise: the moments are
    summed in another order.  Tolerance per field: max(1e-10, 100 s) of the field's max, s the deviation the CPU backend shows
    between two runs whose moments differ by a factor 1 + 2^-52 (printed)."""
    from castro_amd import _lib
    if "dust" not in _CACHE:
        ref, dts, s = R.dust_sensitivity(oracle)
        _CACHE["dust"] = (ref.S_new().numpy().copy(), dts, s, ref.phi_grav().numpy().copy(), ref.poisson_stats())
    want, dts, s, wphi, wst = _CACHE["dust"]
    print("dust collapse with Poisson gravity: s per field =", s)
    tol = np.maximum(1e-10, 100.0 * s)
    c, gdts = R.dust_collapse_run(hydro, _lib.default_params(**R.DUST_PARAMS))
    torch.cuda.synchronize()
    got = c.S_new().cpu().numpy()
    d = MR.field_deviation(got, want)
    print("dust collapse (%s): deviation per field" % hydro.numerics, d, "tolerance", tol)
    assert np.all(d <= tol), (d, tol)
    assert np.allclose(np.array(gdts), np.array(dts), rtol=1e-12, atol=0.0), (gdts, dts)
    assert not c.host_free_ok()
    st = c.poisson_stats()
    assert st["first"]["cycles"] == wst["first"]["cycles"] and st["new"]["cycles"] < st["first"]["cycles"]
    phi = c.phi_grav().cpu().numpy()
    assert np.abs(phi - wphi).max() <= 1e-8 * np.abs(wphi).max()
    # close() gives the plan's device arrays back; a later step makes the plan again
    c.close()
    assert c.poisson.plan is None
    c.step()
    torch.cuda.synchronize()
    assert c.poisson.plan is not None and c.poisson_stats()["new"]["cycles"] >= 1
    c.close()


def test_plan_lifetime(hydro):
    """one plan after a step, none after close(), one again after the next step; the object stays with its driver"""
    import castro_amd
    from castro_amd import _lib
    c, _ = R.dust_collapse_run(hydro, _lib.default_params(**R.DUST_PARAMS), steps=1)
    torch.cuda.synchronize()
    R.assert_plan_lifetime(c)
    with pytest.raises(ValueError, match="one Castro"):
        castro_amd.Castro(R.DUST_N, hydro=hydro, do_grav=True, poisson=c.poisson, **R.DUST_GEOM)
    c.close()

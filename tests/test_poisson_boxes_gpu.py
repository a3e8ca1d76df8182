"""GPU tests of Poisson gravity on refined levels of SEVERAL boxes, for both numerics builds: the masked passes (k_mgb_*), the
level's coarse-fine boundary values (k_phi_cf_boxes) and the gradient against the restatement (tests/poisson_boxes_ref.py), the
tiling identity with the one-box solve, the refusals of the C entry points, and the driver runs of tests/test_poisson_boxes_cpu.py
on the device against the same driver on PoissonBoxesOracleBackend."""
import numpy as np
import pytest
import torch

from tests import monopole_ref as MR
from tests import poisson_boxes_ref as B
from tests import poisson_ref as R

pytestmark = pytest.mark.gpu

_CACHE = {}
SENT = -4.25e33
FOURPI = 4.0 * np.pi
CBOX = ((-1, -1, -1), (16, 16, 16))


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


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _grow(box, n):
    return (tuple(x - n for x in box[0]), tuple(x + n for x in box[1]))


def _sl(box, lo, hi):
    return tuple(slice(lo[d] - box[0][d], hi[d] - box[0][d] + 1) for d in (2, 1, 0))


def _case(name, a=0.3):
    """the restatement of one layout, computed once: random coarse potentials, density in [0.5, 2], a random start on every zone of
    the bounding box; the face values (sentinels in the slots that are not written), the solve and the gradient"""
    key = (name, a)
    if key not in _CACHE:
        plan = B.Plan(B.DX, B.LAYOUTS[name])
        rng = np.random.default_rng(11)
        cbox = B.CRSE_BOX.get(name, CBOX)
        co, cn = rng.normal(size=B.shape_of(cbox)) * 3.0 - 7.0, rng.normal(size=B.shape_of(cbox)) * 3.0 - 7.0
        rho = rng.uniform(0.5, 2.0, size=plan.lev[0].shape)
        start = np.zeros(plan.lev[0].gshape)
        start[1:-1, 1:-1, 1:-1] = rng.normal(size=plan.lev[0].shape) - 7.0
        X = np.full((3,) + B.shape_of(plan.facebox), SENT)
        wrote = B.cf_faces(plan, X, co, cbox, cn, cbox, a)
        phi = start.copy()
        out = B.solve(plan, phi, X, rho, FOURPI)
        _CACHE[key] = dict(plan=plan, cbox=cbox, co=co, cn=cn, rho=rho, start=start, X=X, wrote=wrote, phi=phi, out=out)
    return _CACHE[key]


def _rho_fabs(plan, rho):
    """the density as component 1 of a 3-component FAB per box (the box grown by two, NaN outside the box)"""
    out = []
    for lo, hi in plan.boxes:
        ubox = _grow((lo, hi), 2)
        U = np.full((3,) + B.shape_of(ubox), np.nan)
        U[(1,) + _sl(ubox, lo, hi)] = rho[_sl(plan.bb, lo, hi)]
        out.append((_dev(U), ubox))
    return out


def _device_faces(hydro, c, dplan, a):
    X = torch.full((3,) + B.shape_of(c["plan"].facebox), SENT, dtype=torch.float64, device="cuda")
    hydro.poisson_boxes_cf_bc(dplan, X, c["plan"].facebox, _dev(c["co"][None]), c["cbox"], _dev(c["cn"][None]), c["cbox"], a)
    return X


# ---- 1. the tiling identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tile2", "tile4"])
def test_a_tiling_is_the_one_box_solve(hydro, name):
    """a union that tiles its bounding box BB.  Both builds: the face values of the boxes call are those of poisson_cf_bc on BB,
    bit for bit.  `exact`: phi, norm history and cycle count of poisson_boxes_solve are those of poisson_solve on BB.  `contract`:
    the residual recomputed in float64 meets the stopping tolerance and, on the two-box tiling, the dense bound."""
    from castro_amd import _lib
    c = _case(name)
    plan, bb = c["plan"], c["plan"].bb
    n = plan.lev[0].n
    pbox, fbox = plan.phibox, plan.facebox
    dplan = hydro.poisson_boxes_plan_create(B.DX, plan.boxes)
    geom = _lib.make_geom((32, 32, 32))
    for d in range(3):
        geom.domlo[d], geom.domhi[d] = bb[0][d], bb[1][d]
    oplan = hydro.poisson_plan_create(geom)
    try:
        X = _device_faces(hydro, c, dplan, 0.3)
        one = _dev(c["start"][None])
        hydro.poisson_cf_bc(one, pbox, bb[0], bb[1], _dev(c["co"][None]), CBOX, _dev(c["cn"][None]), CBOX, 0.3)
        gX, gone = _host(X), _host(one)[0]
        assert np.array_equal(_bits(gX), _bits(c["X"])), "the restatement's face values, sentinels in the interior slots"
        pairs = ((gX[0][:-1, :-1, 0], gone[1:-1, 1:-1, 0]), (gX[0][:-1, :-1, -1], gone[1:-1, 1:-1, -1]),
                 (gX[1][:-1, 0, :-1], gone[1:-1, 0, 1:-1]), (gX[1][:-1, -1, :-1], gone[1:-1, -1, 1:-1]),
                 (gX[2][0, :-1, :-1], gone[0, 1:-1, 1:-1]), (gX[2][-1, :-1, :-1], gone[-1, 1:-1, 1:-1]))
        for f, (x, y) in enumerate(pairs):
            assert np.array_equal(_bits(x), _bits(y)), "face %d: the boxes call against poisson_cf_bc on the bounding box" % f
        ubox = _grow(bb, 2)
        U = np.full((3,) + B.shape_of(ubox), np.nan)
        U[(1,) + _sl(ubox, bb[0], bb[1])] = c["rho"]
        wc, wok, wnorm, whist = hydro.poisson_solve(oplan, one, pbox, _dev(U), ubox, 1, FOURPI)
        phi = _dev(c["start"][None])
        cycles, ok, norm, hist = hydro.poisson_boxes_solve(dplan, phi, pbox, X, fbox, _rho_fabs(plan, c["rho"]), 1, FOURPI)
        got, want = _host(phi)[0], _host(one)[0]
        b = FOURPI * c["rho"]
        tol = R.stopping_tolerance(b)
        print("tiling %s (%s): %d cycles (one box %d, restatement %d), final norm %.3g (one box %.3g), tolerance %.3g"
              % (name, hydro.numerics, cycles, wc, c["out"][0], norm, wnorm, tol))
        assert ok and wok and norm <= tol and len(hist) == cycles + 3
        assert np.array_equal(_bits(got[0]), _bits(c["start"][0])) and np.array_equal(_bits(got[:, :, 0]), _bits(c["start"][:, :, 0]))
        if hydro.numerics == "exact":
            assert cycles == wc == c["out"][0]
            assert np.array_equal(_bits(np.array(hist)), _bits(np.array(whist))), (hist, whist)
            assert np.array_equal(_bits(got[1:-1, 1:-1, 1:-1]), _bits(want[1:-1, 1:-1, 1:-1]))
            assert np.array_equal(_bits(got), _bits(c["phi"]))
        else:
            L0 = R.levels(n, B.DX)[0]
            shell = want.copy()
            shell[1:-1, 1:-1, 1:-1] = got[1:-1, 1:-1, 1:-1]                 # the masked solve's phi inside the one-box ghost shell
            rr = np.abs(R.residual(L0, shell, b)).max()
            assert rr <= tol, (rr, tol)
            if name == "tile2":
                dev, bound = R.dense_check(L0, shell, b)
                print("dense check (contract): deviation %.3g, bound %.3g" % (dev, bound))
                assert dev <= bound
    finally:
        hydro.poisson_plan_destroy(dplan)
        hydro.poisson_plan_destroy(oplan)


# ---- 2. the irregular layouts against the restatement -------------------------------------------------------------------------------
def _layout_against_the_restatement(hydro, name, a):
    """Face values: the restatement's bits in both builds, every slot that is not a boundary face of the union keeps its sentinel.
    Solve: `exact` gives phi (uncovered zones and ghost zones keep their bits), norm history and cycle count of the restatement;
    `contract` meets the stopping rule on the float64 residual of the masked operator.  g per box: `exact` the restatement's
    bits from the device's phi, `contract` within 8 * 2^-52 of the magnitudes; NaN outside the box."""
    c = _case(name, a)
    plan = c["plan"]
    pbox, fbox = plan.phibox, plan.facebox
    dplan = hydro.poisson_boxes_plan_create(B.DX, plan.boxes)
    try:
        X = _device_faces(hydro, c, dplan, a)
        gX = _host(X)
        assert np.all(c["X"][~c["wrote"]] == SENT) and np.all(c["X"][c["wrote"]] != SENT)
        d = _bits(gX) != _bits(c["X"])
        assert not d.any(), "%d of %d face slots differ (%d of them slots that must not be written)" % (
            int(d.sum()), d.size, int((d & ~c["wrote"]).sum()))
        phi = _dev(c["start"][None])
        cycles, ok, norm, hist = hydro.poisson_boxes_solve(dplan, phi, pbox, X, fbox, _rho_fabs(plan, c["rho"]), 1, FOURPI)
        got = _host(phi)[0]
        wc, wok, wnorm, whist = c["out"]
        cov = plan.covered()
        b = np.where(cov, FOURPI * c["rho"], 0.0)
        tol = R.stopping_tolerance(b[cov])
        print("layout %s a = %g (%s): %d cycles (restatement %d), final norm %.3g, tolerance %.3g"
              % (name, a, hydro.numerics, cycles, wc, norm, tol))
        assert wok and ok and norm <= tol and len(hist) == cycles + 3
        keep = np.ones(got.shape, dtype=bool)
        keep[1:-1, 1:-1, 1:-1] = ~cov
        assert np.array_equal(_bits(got[keep]), _bits(c["start"][keep])), "uncovered zones and ghost zones keep the bits they were given"
        if hydro.numerics == "exact":
            assert cycles == wc
            assert np.array_equal(_bits(np.array(hist)), _bits(np.array(whist))), (hist, whist)
            assert np.array_equal(_bits(got), _bits(c["phi"]))
        else:
            rr = B.masked_residual64(plan, got, c["X"], b)
            assert rr <= tol, (rr, tol)
        gravs = [(torch.full((3,) + B.shape_of(_grow(bx, 1)), float("nan"), dtype=torch.float64, device="cuda"), _grow(bx, 1))
                 for bx in plan.boxes]
        hydro.grad_phi_to_grav_boxes(dplan, phi, pbox, X, fbox, gravs)
        mag = np.zeros((3,) + plan.lev[0].shape)
        wg = B.grad_phi(plan, got, c["X"], mag)
        for (G, gbox), (lo, hi) in zip(gravs, plan.boxes):
            gg = _host(G)
            inner = gg[:, 1:-1, 1:-1, 1:-1]
            outside = np.ones(gg.shape, dtype=bool)
            outside[:, 1:-1, 1:-1, 1:-1] = False
            assert np.isnan(gg[outside]).all(), "g keeps NaN outside the valid zones of its box"
            w = wg[(slice(None),) + _sl(plan.bb, lo, hi)]
            if hydro.numerics == "exact":
                assert np.array_equal(_bits(inner), _bits(w)), (lo, hi)
            else:
                assert np.all(np.abs(inner - w) <= 8.0 * R.U52 * mag[(slice(None),) + _sl(plan.bb, lo, hi)]), (lo, hi)
    finally:
        hydro.poisson_plan_destroy(dplan)


@pytest.mark.parametrize("a", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("name", ["ell", "edge", "disjoint", "unequal"])
def test_layout_against_the_restatement(hydro, name, a):
    _layout_against_the_restatement(hydro, name, a)


def test_layout_with_a_bottom_solve_of_three_trips_against_the_restatement(hydro):
    """two boxes aligned to 2 only: the bottom solve runs on level 1, 15 x 16 x 17 of the bounding box with 78 % of it covered --
    2176 x-pairs per colour for the 1024 threads of k_mgb_bottom, three trips with a barrier after each colour.  The assertions
    of the other layouts, at a = 0.3."""
    c = _case("wide_bottom", 0.3)
    assert [L.n for L in c["plan"].lev] == [(30, 32, 34), (15, 16, 17)] and c["out"][1] and c["out"][0] >= 3
    _layout_against_the_restatement(hydro, "wide_bottom", 0.3)


# ---- 3. single passes on the two coarsest levels of the ell: boxes 2 and 1 zones wide ------------------------------------------------
@pytest.mark.parametrize("level", [1, 2])
def test_single_passes_on_the_coarse_levels_of_the_ell(hydro, level):
    """`exact`: the restatement's bits.  `contract`: a fused multiply-add moves a result by less than one rounding per fused pair;
    the passes are granted 8 * 2^-52 of a bound on the sum of the magnitudes of their terms -- smoother (2 (cx + cy + cz) max|p| +
    |b|) / cdiag, residual |b| + 4 (cx + cy + cz) max|p|, restriction max|r|; the prolongation (one addition) and the norms
    (maxima) are the same bits in both builds.  Zones that are not covered keep their sentinel."""
    from castro_amd import _lib
    plan = B.Plan(B.DX, B.LAYOUTS["ell"])
    assert [L.n for L in plan.lev] == [(16, 16, 8), (8, 8, 4), (4, 4, 2)]
    exact = hydro.numerics == "exact"
    L, fl, lo = plan.lev[level], plan.flags[level], plan.lo[level]
    box = (lo, tuple(lo[d] + L.n[d] - 1 for d in range(3)))
    cov = plan.covered(level)
    rng = np.random.default_rng(17 + level)
    P0 = rng.normal(size=L.gshape) * 2.0 - 3.0
    Bv = rng.normal(size=L.shape) * 40.0
    csum = (L.cx + L.cy) + L.cz
    pmax = np.abs(P0).max()
    dplan = hydro.poisson_boxes_plan_create(B.DX, plan.boxes)

    def close(got, want, bound, what):
        if exact:
            assert np.array_equal(_bits(got), _bits(want)), what
        else:
            assert np.all(np.abs(got - want) <= 8.0 * R.U52 * bound), (what, np.abs(got - want).max())

    try:
        for colour in (0, 1):
            want = P0.copy()
            B.smooth(L, fl, want, Bv, None, colour)
            Pd = _dev(P0[None])
            hydro.poisson_boxes_level_op(dplan, _lib.MG_SMOOTH, level, (Pd, _grow(box, 1)), (_dev(Bv[None]), box), colour=colour)
            got = _host(Pd)[0]
            sel = np.zeros(L.gshape, dtype=bool)
            sel[1:-1, 1:-1, 1:-1] = cov & (B._parity(L) == colour)
            assert sel.sum() > 0 and np.array_equal(_bits(got[~sel]), _bits(P0[~sel])), "only covered zones of the colour are written"
            close(got[sel], want[sel], (2.0 * csum * pmax + np.abs(Bv).max()) / L.cdiag, "smooth %d" % colour)
        want = B.residual(L, fl, P0, Bv, None, np.full(L.shape, SENT))
        Rd = torch.full((1,) + L.shape, SENT, dtype=torch.float64, device="cuda")
        hydro.poisson_boxes_level_op(dplan, _lib.MG_RESIDUAL, level, (_dev(P0[None]), _grow(box, 1)), (_dev(Bv[None]), box), (Rd, box))
        got = _host(Rd)[0]
        assert np.all(got[~cov] == SENT)
        close(got[cov], want[cov], np.abs(Bv).max() + 4.0 * csum * pmax, "residual")
        out = torch.zeros(2, dtype=torch.float64, device="cuda")
        hydro.poisson_boxes_level_op(dplan, _lib.MG_NORM, level, (_dev(want[None]), box), out=out)
        assert tuple(_host(out)) == B.norm(want, fl), "the sentinels of the uncovered zones (the largest magnitudes) do not enter"
        if level == 1:
            # from level 1 to level 2 and back
            L2, fl2, lo2 = plan.lev[2], plan.flags[2], plan.lo[2]
            box2 = (lo2, tuple(lo2[d] + L2.n[d] - 1 for d in range(3)))
            Rf = np.where(cov, rng.normal(size=L.shape), np.nan)
            wB, wP = np.full(L2.shape, SENT), np.full(L2.gshape, SENT)
            B.restrict(np.nan_to_num(Rf), fl2, wB, wP)
            Bd = torch.full((1,) + L2.shape, SENT, dtype=torch.float64, device="cuda")
            Pd = torch.full((1,) + L2.shape, SENT, dtype=torch.float64, device="cuda")
            hydro.poisson_boxes_level_op(dplan, _lib.MG_RESTRICT, 1, (_dev(Rf[None]), box), (Bd, box2), (Pd, box2))
            gB, gP = _host(Bd)[0], _host(Pd)[0]
            c2 = plan.covered(2)
            assert np.all(gB[~c2] == SENT) and np.all(gP[~c2] == SENT) and np.all(gP[c2] == 0.0)
            close(gB[c2], wB[c2], np.nanmax(np.abs(Rf)), "restrict")
            PC = np.where(c2, rng.normal(size=L2.shape), np.nan)
            PCg = np.zeros(L2.gshape)
            PCg[1:-1, 1:-1, 1:-1] = np.nan_to_num(PC)
            want = P0.copy()
            B.prolong(PCg, want, fl)
            Fd = _dev(P0[None, 1:-1, 1:-1, 1:-1])
            hydro.poisson_boxes_level_op(dplan, _lib.MG_PROLONG, 1, (_dev(PC[None]), box2), (Fd, box))
            assert np.array_equal(_bits(_host(Fd)[0]), _bits(want[1:-1, 1:-1, 1:-1])), "prolong: NaN of an uncovered coarse zone is never read"
    finally:
        hydro.poisson_plan_destroy(dplan)


def test_single_passes_on_level_0_of_the_ell_with_face_values(hydro):
    """the smoother (both colours) and the residual on level 0 (bounding box 16 x 16 x 8) with a random face array that holds NaN
    in every slot no flagged face owns -- a pass that reads a face value where no flag asks for it, or a neighbour's value where a
    flag asks for the face's, shows.  The rule of the passes on the coarse levels: `exact` the restatement's bits, `contract`
    8 * 2^-52 of a bound on the sum of the magnitudes of the terms.  With m = max(|p|, |f|) and at most one flagged face per
    direction (the boxes are 8 zones wide) a flagged neighbour is 2 f in the smoother and 2 f - p in the residual: smoother
    (3 (cx + cy + cz) m + |b|) / cdiag (the diagonal only grows), residual |b| + 6 (cx + cy + cz) m.  Zones that are not covered,
    and the zones of the other colour, keep their bits."""
    from castro_amd import _lib
    plan = B.Plan(B.DX, B.LAYOUTS["ell"])
    L, fl = plan.lev[0], plan.flags[0]
    assert L.n == (16, 16, 8)
    exact = hydro.numerics == "exact"
    box, fbox = plan.bb, plan.facebox
    cov = plan.covered()
    rng = np.random.default_rng(23)
    P0 = rng.normal(size=L.gshape) * 2.0 - 3.0
    Bv = rng.normal(size=L.shape) * 40.0
    nz, ny, nx = L.shape
    owned = np.zeros((3,) + B.shape_of(fbox), dtype=bool)
    for d in range(3):
        for side in (0, 1):
            off = [0, 0, 0]
            off[2 - d] = side
            owned[d][off[0]:off[0] + nz, off[1]:off[1] + ny, off[2]:off[2] + nx] |= (fl & B.face_bit(d, side)) != 0
    assert owned.any() and not owned.all()
    X = np.where(owned, rng.normal(size=owned.shape) * 2.0 - 3.0, np.nan)
    csum = (L.cx + L.cy) + L.cz
    pmax = max(np.abs(P0).max(), np.abs(X[owned]).max())
    dplan = hydro.poisson_boxes_plan_create(B.DX, plan.boxes)

    def close(got, want, bound, what):
        assert np.isfinite(want).all(), what
        if exact:
            assert np.array_equal(_bits(got), _bits(want)), what
        else:
            assert np.all(np.abs(got - want) <= 8.0 * R.U52 * bound), (what, np.abs(got - want).max())

    try:
        Xd = (_dev(X), fbox)
        for colour in (0, 1):
            want = P0.copy()
            B.smooth(L, fl, want, Bv, X, colour)
            Pd = _dev(P0[None])
            hydro.poisson_boxes_level_op(dplan, _lib.MG_SMOOTH, 0, (Pd, _grow(box, 1)), (_dev(Bv[None]), box), faces=Xd, colour=colour)
            got = _host(Pd)[0]
            sel = np.zeros(L.gshape, dtype=bool)
            sel[1:-1, 1:-1, 1:-1] = cov & (B._parity(L) == colour)
            assert sel.sum() > 0 and np.array_equal(_bits(got[~sel]), _bits(P0[~sel])), "only covered zones of the colour are written"
            close(got[sel], want[sel], (3.0 * csum * pmax + np.abs(Bv).max()) / L.cdiag, "smooth %d" % colour)
        want = B.residual(L, fl, P0, Bv, X, np.full(L.shape, SENT))
        Rd = torch.full((1,) + L.shape, SENT, dtype=torch.float64, device="cuda")
        hydro.poisson_boxes_level_op(dplan, _lib.MG_RESIDUAL, 0, (_dev(P0[None]), _grow(box, 1)), (_dev(Bv[None]), box), (Rd, box), faces=Xd)
        got = _host(Rd)[0]
        assert np.all(got[~cov] == SENT)
        close(got[cov], want[cov], np.abs(Bv).max() + 6.0 * csum * pmax, "residual")
    finally:
        hydro.poisson_plan_destroy(dplan)


# ---- 4. the refusals of the C entry points ------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry(hydro):
    """each refusal returns its error code (a RuntimeError that names it) before anything is launched: the arrays keep their bits"""
    cube = B._cube
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.poisson_boxes_plan_create(B.DX, [cube((8, 8, 8)), cube((12, 8, 8))])              # overlapping boxes
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.poisson_boxes_plan_create(B.DX, [cube((8, 8, 8)), ((17, 8, 8), (23, 15, 15))])    # a box not aligned to 2
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.poisson_boxes_plan_create(B.DX, [cube((8, 8, 8)), ((16, 8, 8), (22, 15, 15))])
    with pytest.raises(RuntimeError, match="unsupported"):                                      # 36^3 aligned to 2: 18^3 > 4096 zones
        hydro.poisson_boxes_plan_create(B.DX, [((2, 2, 2), (5, 5, 5)), ((34, 34, 34), (37, 37, 37))])
    c = _case("ell")
    plan = c["plan"]
    pbox, fbox = plan.phibox, plan.facebox
    dplan = hydro.poisson_boxes_plan_create(B.DX, plan.boxes)
    try:
        X = torch.full((3,) + B.shape_of(fbox), SENT, dtype=torch.float64, device="cuda")
        O, N = _dev(c["co"][None]), _dev(c["cn"][None])
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.poisson_boxes_cf_bc(dplan, X, fbox, O, CBOX, N, CBOX, float("nan"))
        small = ((4, 4, 4), (11, 11, 7))                        # the coarsened bounding box, not grown by one: the slopes read beyond it
        Os = _dev(c["co"][(None,) + _sl(CBOX, *small)])
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.poisson_boxes_cf_bc(dplan, X, fbox, Os, small, N, CBOX, 0.3)
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.poisson_boxes_cf_bc(dplan, X, fbox, O, CBOX, Os, small, 0.3)
        with pytest.raises(RuntimeError, match="bad argument"):  # a face array over the bounding box only: no slot for the high faces
            hydro.poisson_boxes_cf_bc(dplan, X[:, :-1, :-1, :-1].contiguous(), plan.bb, O, CBOX, N, CBOX, 0.3)
        phi = _dev(c["start"][None])
        rhos = _rho_fabs(plan, c["rho"])
        with pytest.raises(RuntimeError, match="bad argument"):  # phi without its ghost zone
            hydro.poisson_boxes_solve(dplan, phi[:, 1:-1, 1:-1, 1:-1].contiguous(), plan.bb, X, fbox, rhos, 1, FOURPI)
        with pytest.raises(RuntimeError, match="bad argument"):  # a density FAB per box
            hydro.poisson_boxes_solve(dplan, phi, pbox, X, fbox, rhos[:2], 1, FOURPI)
        with pytest.raises(RuntimeError, match="bad argument"):  # ... that holds its box
            hydro.poisson_boxes_solve(dplan, phi, pbox, X, fbox, [rhos[1], rhos[0], rhos[2]], 1, FOURPI)
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.poisson_boxes_solve(dplan, phi, pbox, X, fbox, rhos, 3, FOURPI)
        with pytest.raises(RuntimeError, match="bad argument"):  # the one-box entry point refuses the plan of a union
            hydro.poisson_solve(dplan, phi, pbox, rhos[0][0], rhos[0][1], 1, FOURPI)
        gravs = [(torch.full((3,) + B.shape_of(bx), SENT, dtype=torch.float64, device="cuda"), bx) for bx in plan.boxes]
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.grad_phi_to_grav_boxes(dplan, phi, pbox, X, fbox, gravs[::-1])
        assert np.all(_host(X) == SENT) and np.array_equal(_bits(_host(phi)[0]), _bits(c["start"]))
        assert all(np.all(_host(G) == SENT) for G, _ in gravs)
    finally:
        hydro.poisson_plan_destroy(dplan)


# ---- 5. the driver ------------------------------------------------------------------------------------------------------------------
def _compare(hydro, what, got, want, s, gdts, dts):
    """`exact`: S_new, phi and g of every box of every level bit for bit, equal dts.  `contract`: per field and level within
    max(1e-10, 100 s) of the field's max, s the deviation the CPU backend shows between two runs whose moments differ by a factor
    1 + 2^-52; phi and g within 1e-8 of their maxima; dts at rtol 1e-12"""
    for l, ((wS, wphi, wcov, wg), (gS, gphi, gcov, gg)) in enumerate(zip(want, got)):
        assert len(gS) == len(wS) and np.array_equal(gcov, wcov)
        dS = np.max([MR.field_deviation(x, y) for x, y in zip(gS, wS)], axis=0)
        gmax = max(np.abs(y).max() for y in wg)
        dphi = np.abs(gphi - wphi)[wcov].max() / np.abs(wphi[wcov]).max()
        dg = max(np.abs(x - y).max() for x, y in zip(gg, wg)) / gmax
        print("%s (%s) level %d, %d boxes: state deviation" % (what, hydro.numerics, l, len(gS)), dS, "s", s[l], "phi %.3g g %.3g" % (dphi, dg))
        if hydro.numerics == "exact":
            for n, (x, y) in enumerate(zip(gS, wS)):
                assert np.array_equal(_bits(x), _bits(y)), "S_new of box %d of level %d" % (n, l)
            assert np.array_equal(_bits(gphi), _bits(wphi)), "phi of level %d" % l
            for n, (x, y) in enumerate(zip(gg, wg)):
                assert np.array_equal(_bits(x), _bits(y)), "g of box %d of level %d" % (n, l)
        else:
            tol = np.maximum(1e-10, 100.0 * s[l])
            assert np.all(dS <= tol), (l, dS, tol)
            assert dphi <= 1e-8 and dg <= 1e-8, (l, dphi, dg)
    print("dts", gdts, dts)
    if hydro.numerics == "exact":
        assert gdts == dts
    else:
        assert np.allclose(np.array(gdts), np.array(dts), rtol=1e-12, atol=0.0), (gdts, dts)


def _reference(oracle, key, run, *args):
    if ("ref", key) not in _CACHE:
        fields, ref, s = B.sensitivity(lambda mk, *a: run(mk, oracle.default_params(**R.DUST_PARAMS), *a), *args)
        _CACHE[("ref", key)] = (fields, ref[1:], s, list(ref[0].gravity.solve_log))
    return _CACHE[("ref", key)]


@pytest.mark.parametrize("case", ["ell", "nested"])
def test_dust_collapse_on_levels_of_several_boxes_against_the_cpu_backend(hydro, oracle, case):
    """the dust collapse on 16^3 with the three boxes of the ell as level 1, and with two boxes nested in them as level 2: two
    coarse steps on the device against the same driver on PoissonBoxesOracleBackend"""
    import castro_amd
    from castro_amd import _lib
    want, (dts,), s, wlog = _reference(oracle, case, B.dust_boxes_run, case)
    a, gdts = B.dust_boxes_run(lambda: castro_amd.HipHydro(0, numerics=hydro.numerics), _lib.default_params(**R.DUST_PARAMS), case)
    torch.cuda.synchronize()
    assert [len(lev.boxes) for lev in a.lev] == ([1, 3] if case == "ell" else [1, 3, 2])
    assert a.gravity.solve_log == wlog
    _compare(hydro, "dust collapse %s" % case, B.level_fields(a), want, s, gdts, dts)
    a.close()
    assert all(ent["plan"] is None for ent in a.gravity._lev.values())


def test_tagged_and_clustered_level_against_the_cpu_backend(hydro, oracle):
    """refine= + cluster=True with a density-gradient tag, one step, a regrid with a wider buffer, one step: level 1 is a union of
    several boxes before and after the regrid, on the device as on the CPU backend, and its solves converge"""
    import castro_amd
    from castro_amd import _lib
    want, (dts, (first, second)), s, wlog = _reference(oracle, "clustered", B.clustered_run)
    assert len(first) > 1 and len(second) > 1 and first != second, "the reference run itself must yield levels of several boxes"
    a, gdts, (gfirst, gsecond) = B.clustered_run(lambda: castro_amd.HipHydro(0, numerics=hydro.numerics),
                                                 _lib.default_params(**R.DUST_PARAMS))
    torch.cuda.synchronize()
    assert gfirst == first and gsecond == second and len(a.lev[1].boxes) == len(second) > 1
    assert a.gravity.solve_log == wlog
    st = a.poisson_stats(1)
    print("clustered level 1: %d then %d boxes, cycles first / new %d / %d" % (len(first), len(second), st["first"]["cycles"], st["new"]["cycles"]))
    assert st["new"]["norm"] <= max(1e-10 * st["new"]["history"][0], 1e-10 * st["new"]["history"][1])
    _compare(hydro, "clustered dust ball", B.level_fields(a), want, s, gdts, dts)
    a.close()
    assert all(ent["plan"] is None for ent in a.gravity._lev.values())

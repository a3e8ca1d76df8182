"""GPU tests ABOVE the grid caps of the reduction kernels, for both numerics builds: the multigrid norm beyond MG_NORM_MAX_WG
workgroups (one box and a union of boxes), the multipole moments with more than one zone per thread, the integrated quantities
and the checkpoint pack / min-max / unpack with `iters` doubled once and twice.  The shapes are those of tests/grid_caps.py, the
smallest that cross each cap (tests/test_grid_caps_cpu.py asserts that they do); the bottom solves of more than one trip and the
moments at the order cap are cases of tests/test_poisson_gpu.py and tests/test_poisson_boxes_gpu.py.

References: numpy maxima and tests/poisson_ref.py, tests/poisson_boxes_ref.py for the multigrid, R.moments with its derived bound
for the moments, int64 sums of a state whose float64 sums are exact in any order for the integrated quantities, torch slicing
and amin / amax for the pack.  Everything but the moments is compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import grid_caps as G
from tests import poisson_boxes_ref as B
from tests import poisson_ref as R
from tests.test_checkpoint_gpu import _eq, _fab, _valid
from tests.test_poisson_gpu import DX, FOURPIG, _bits, _dev
from tests.util import physical_state

pytestmark = pytest.mark.gpu

_CACHE = {}
NAN = float("nan")


@pytest.fixture(scope="module", params=["exact", "contract"])
def hydro(request):
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=request.param)
    yield h
    h.close()


def _same(got, want):
    """two tuples of doubles: the same bits, a NaN equal to a NaN"""
    return all((np.isnan(g) and np.isnan(w)) or (g == w and np.signbit(g) == np.signbit(w)) for g, w in zip(got, want))


# ---- 1. the multigrid norm beyond 1024 workgroups, one box ---------------------------------------------------------------------------
def _one_box_geom():
    from castro_amd import _lib
    n = G.MG_NORM_ONE_BOX
    return _lib.make_geom(n, prob_hi=tuple(n[d] * DX[d] for d in range(3)))


def test_norm_of_one_box_beyond_the_workgroup_cap(hydro):
    """64 x 64 x 80 = 1280 workgroups' worth of zones on 1024: the zones with k >= 64 are taken on the second trip of the
    grid-stride loop, and k_mg_norm_final reduces 1024 live rows.  The FAB holds one ghost zone of NaN."""
    from castro_amd import _lib
    n = G.MG_NORM_ONE_BOX
    shape = (n[2], n[1], n[0])
    assert _lib.poisson_level_extents(n)[-1] == (4, 4, 5)
    plan = hydro.poisson_plan_create(_one_box_geom())
    rng = np.random.default_rng(101)

    def norm(x):
        F = np.full(tuple(s + 2 for s in shape), np.nan)
        F[1:-1, 1:-1, 1:-1] = x
        out = torch.full((2,), 777.0, dtype=torch.float64, device="cuda")
        hydro.poisson_level_op(plan, _lib.MG_NORM, 0, (_dev(F[None]), ((-1, -1, -1), n)), out=out)
        torch.cuda.synchronize()
        return tuple(float(v) for v in out.cpu().numpy())

    try:
        # (a) a random normal field
        x = rng.normal(size=shape)
        assert _same(norm(x), (np.abs(x).max(), x.max()))
        # (b) the largest |x|, negative, in the last zone; the largest x at another zone of the second trip
        x = rng.uniform(-1.0, 1.0, size=shape)
        x[79, 63, 63] = -7.5
        x[70, 5, 9] = 3.25
        assert (np.abs(x).max(), x.max()) == (7.5, 3.25) and _same(norm(x), (7.5, 3.25))
        # the maximum in the first and the last zone of either trip: rows 0 and 1023 of the workspace, both ends of the loop
        for k, j, i in ((0, 0, 0), (63, 63, 63), (64, 0, 0), (79, 63, 63)):
            y = x.copy()
            y[k, j, i] = 9.0
            assert _same(norm(y), (9.0, 9.0)), (k, j, i)
        # (c) one NaN on the second trip and nowhere else
        y = x.copy()
        y[66, 1, 2] = np.nan
        got = norm(y)
        assert np.isnan(got[0]) and np.isnan(got[1]), got
        # (d) an all-negative field: the -inf the idle rows and lanes start from does not leak, nor does the 0 of max |x|
        x = -rng.uniform(1.0, 2.0, size=shape)
        x[72, 40, 33] = -0.5                                     # the largest value, on the second trip
        got = norm(x)
        assert _same(got, (np.abs(x).max(), -0.5)) and got[1] < 0.0
    finally:
        hydro.poisson_plan_destroy(plan)


def _solve_reference(dx):
    key = ("solve", dx)
    if key not in _CACHE:
        from tests.test_poisson_cpu import _mg_case
        rho, phi = _mg_case(G.MG_NORM_ONE_BOX)
        start = phi.copy()
        out = R.solve(G.MG_NORM_ONE_BOX, dx, phi, rho, FOURPIG)
        _CACHE[key] = (rho, start, phi, out)
    return _CACHE[key]


def test_solve_of_one_box_beyond_the_norm_cap(hydro):
    """one solve on 64 x 64 x 80, five levels down to (4, 4, 5): every norm of the history is taken by the capped grid.  `exact`:
    cycle count, the whole norm history and phi are the restatement's bits.  `contract`: the residual recomputed in float64 meets
    the stopping tolerance."""
    n = G.MG_NORM_ONE_BOX
    geom = _one_box_geom()
    dx = tuple(geom.dx[d] for d in range(3))
    rho, start, wphi, (wcycles, wok, wnorm, whist) = _solve_reference(dx)
    assert wok and wcycles >= 3, "the history holds at least three V-cycle norms"
    U = np.full((3, n[2] + 4, n[1] + 4, n[0] + 4), np.nan)
    U[1, 2:-2, 2:-2, 2:-2] = rho
    plan = hydro.poisson_plan_create(geom)
    try:
        P = _dev(start[None])
        cycles, ok, norm, hist = hydro.poisson_solve(plan, P, ((-1, -1, -1), n), _dev(U), ((-2, -2, -2), tuple(v + 1 for v in n)), 1, FOURPIG)
        torch.cuda.synchronize()
        got = P.cpu().numpy()[0]
    finally:
        hydro.poisson_plan_destroy(plan)
    shell = np.ones(got.shape, dtype=bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(_bits(got[shell]), _bits(start[shell])), "the boundary values are not written"
    b = FOURPIG * rho
    tol = R.stopping_tolerance(b)
    print("solve %s (%s): %d cycles (restatement %d), final norm %.3g, tolerance %.3g" % (n, hydro.numerics, cycles, wcycles, norm, tol))
    assert ok and norm <= tol and len(hist) == cycles + 3 and cycles >= 3
    assert hist[0] == np.abs(b).max() and hist[1] == b.max(), "the norms of the right-hand side: maxima, the same bits in both builds"
    if hydro.numerics == "exact":
        assert cycles == wcycles
        assert np.array_equal(_bits(np.array(hist)), _bits(np.array(whist))), (hist, whist)
        assert np.array_equal(_bits(got), _bits(wphi))
    else:
        rr = np.abs(R.residual(R.levels(n, dx)[0], got, b)).max()
        assert rr <= tol, (rr, tol)


# ---- 2. the same norm on a union of boxes -----------------------------------------------------------------------------------------
def test_norm_of_a_union_beyond_the_workgroup_cap(hydro):
    """two boxes in a bounding box of 64 x 64 x 80, 80 % covered; the uncovered zones (i >= 32, k >= 48) reach into the second
    trip.  Level 0 only, against B.norm over the covered zones."""
    from castro_amd import _lib
    if "union" not in _CACHE:
        _CACHE["union"] = B.Plan(B.DX, G.MG_NORM_UNION)
    plan = _CACHE["union"]
    fl, cov = plan.flags[0], plan.covered()
    assert plan.lev[0].n == (64, 64, 80) and int(cov.sum()) * 5 == cov.size * 4
    assert not cov[70, 10, 40] and cov[70, 10, 5] and cov[79, 63, 31] and not cov[79, 63, 63]
    dplan = hydro.poisson_boxes_plan_create(B.DX, plan.boxes)
    rng = np.random.default_rng(102)

    def norm(x):
        out = torch.full((2,), 777.0, dtype=torch.float64, device="cuda")
        hydro.poisson_boxes_level_op(dplan, _lib.MG_NORM, 0, (_dev(x[None]), plan.bb), out=out)
        torch.cuda.synchronize()
        return tuple(float(v) for v in out.cpu().numpy())

    try:
        x = rng.normal(size=plan.lev[0].shape)
        want = B.norm(x, fl)
        assert _same(norm(x), want)
        y = x.copy()
        y[70, 10, 40] = -1.0e30                                  # the largest magnitude of all, in an uncovered zone
        y[79, 63, 63] = 1.0e30
        assert _same(norm(y), want), "uncovered zones of the second trip are ignored"
        y[70, 10, 40] = np.nan
        y[79, 63, 63] = np.nan
        assert _same(norm(y), want), "a NaN in an uncovered zone is ignored"
        # the maximum in the first and the last covered zone of either trip
        for k, j, i in ((0, 0, 0), (63, 63, 31), (64, 0, 0), (79, 63, 31)):
            z = y.copy()
            assert cov[k, j, i]
            z[k, j, i] = 9.0
            assert _same(norm(z), (9.0, 9.0)), (k, j, i)
        y[70, 10, 5] = -50.0                                    # covered zones of the second trip: seen
        y[79, 63, 31] = 40.0
        assert _same(norm(y), (50.0, 40.0)) and _same(B.norm(y, fl), (50.0, 40.0))
        y[79, 63, 31] = np.nan
        got = norm(y)
        assert np.isnan(got[0]) and np.isnan(got[1]), "a NaN in a covered zone of the second trip gives NaN"
    finally:
        hydro.poisson_plan_destroy(dplan)


# ---- 4. multipole moments with two zones per thread -------------------------------------------------------------------------------
def _mp_boxes():
    """the domain (72, 64, 64) as three boxes cut at odd x, on FABs with 1, 4 and 3 NaN ghost zones; on the middle box a mask with
    scattered zeros and a block of zeros at its highest k, NaN density under every zero"""
    if "mp" not in _CACHE:
        c = G.MP_LARGE
        n = c["n_cell"]
        rng = np.random.default_rng(41)
        out = []
        for (x0, x1), ng in zip(c["cuts"], c["ghosts"]):
            lo, hi = (x0, 0, 0), (x1, n[1] - 1, n[2] - 1)
            ext = tuple(hi[d] - lo[d] + 1 for d in range(3))
            U = physical_state(rng, lo, hi, jump=False)
            mask = None
            if ng == 4:
                mask = (rng.uniform(size=ext[::-1]) > 0.15).astype(np.uint8)
                mask[-3:] = 0
                assert mask[:-3].min() == 0 and mask[:-3].max() == 1
                U[0][mask == 0] = np.nan
            F = np.full((8,) + tuple(e + 2 * ng for e in ext[::-1]), np.nan)
            F[:, ng:ng + ext[2], ng:ng + ext[1], ng:ng + ext[0]] = U
            fbox = (tuple(x - ng for x in lo), tuple(x + ng for x in hi))
            out.append((U[0].copy(), lo, hi, mask, F, fbox))
        _CACHE["mp"] = out
    return _CACHE["mp"]


def test_multipole_moments_with_two_zones_per_thread(hydro):
    """294 912 zones in three boxes: 1152 workgroups at one zone per thread, so `iters` = 2 and 576 workgroups per order; the
    second zone of a thread is masked (skipped, not the end of the loop), past the box (the end), or live"""
    from castro_amd import _lib
    c = G.MP_LARGE
    geom = _lib.make_geom(c["n_cell"], prob_hi=c["prob_hi"])
    mp = _lib.make_multipole(geom, c["center"], c["lnum"])
    boxes = _mp_boxes()
    assert sum(b[0].size for b in boxes) == 294912
    if "mp_ref" not in _CACHE:
        _CACHE["mp_ref"] = R.moments([(rho, lo, mask) for rho, lo, hi, mask, F, fbox in boxes], geom, mp)
    want, bound = _CACHE["mp_ref"]
    dev = [(_dev(F), None if mask is None else _dev(mask)) for _, _, _, mask, F, _ in boxes]
    table = hydro.make_diag_boxes([(b[1], b[2], (d[0], b[5]), d[1]) for b, d in zip(boxes, dev)])
    lnum = c["lnum"]
    n = 3 * (lnum + 1) ** 2

    def call(stream=None):
        out = torch.full((n,), NAN, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        hydro.multipole_moments_mf(table, geom, mp, out, stream=stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    got = call()
    err = np.abs(got - want)
    live = bound > 0
    print("moments of 294912 zones, lnum %d (%s): worst deviation / bound = %.3g over %d moments, worst bound / |q| = %.3g"
          % (lnum, hydro.numerics, float((err[live] / bound[live]).max()), int(live.sum()), float((bound[live] / np.abs(want[live])).max())))
    assert live.sum() == (lnum + 1) + lnum * (lnum + 1)
    assert np.all(got[~live] == 0.0), "entries the loop nest does not reach are zero"
    assert np.isfinite(got).all() and np.all(err <= bound), (err[live] / bound[live])
    assert np.array_equal(_bits(call()), _bits(got)), "two calls: the same bits"
    assert np.array_equal(_bits(call(stream=torch.cuda.Stream())), _bits(got)), "another stream: the same bits"


# ---- 5. integrated quantities with iters = 8 --------------------------------------------------------------------------------------
def _diag_state():
    """an integer state whose 14 sums are exact in any order, the two masks' worth of int64 sums, and the units they are in.
    rho in {1, 2, 4}, momenta in +-1..8, (rho e), (rho E) and the species in 1..16 on zones whose widths are powers of two
    around the centre (0.5, 0.5, 0.5): every term of diag_add, every product inside it (fused or not) and every partial sum is
    a dyadic rational of fewer than 53 bits.  Coordinates in units of 2^-9, the zone volume is 2^-23."""
    if "diag" in _CACHE:
        return _CACHE["diag"]
    from castro_amd import _lib as L
    c = G.DIAG_LARGE
    lo, (nx, ny, nz) = c["lo"], c["ext"]
    shape = (nz, ny, nx)
    rng = np.random.default_rng(51)
    S = np.ones((8,) + shape, dtype=np.int8)
    S[0] = 1 << rng.integers(0, 3, size=shape)
    for m in (1, 2, 3):
        S[m] = rng.integers(1, 9, size=shape) * (2 * rng.integers(0, 2, size=shape) - 1)
    for m in (4, 5, 7):
        S[m] = rng.integers(1, 17, size=shape)
    mask = (rng.uniform(size=shape) > 0.1).astype(np.uint8)
    mask[-2:] = 0                                                # a slab at the highest k
    assert mask[:-2].min() == 0 and mask[:-2].max() == 1
    # zone centres and their distance from the centre in units of 2^-9 (dx = dz = 2^-8, dy = 2^-7)
    X = (2 * (lo[0] + np.arange(nx, dtype=np.int64)) + 1).reshape(1, 1, nx)
    Y = (4 * (lo[1] + np.arange(ny, dtype=np.int64)) + 2).reshape(1, ny, 1)
    Z = (2 * (lo[2] + np.arange(nz, dtype=np.int64)) + 1).reshape(nz, 1, 1)
    rho, mx, my, mz, eden, eint, rx = (S[m].astype(np.int64) for m in (0, 1, 2, 3, 4, 5, 7))
    terms, unit = [None] * 14, np.zeros(14)
    for m, t in ((L.DIAG_MASS, rho), (L.DIAG_XMOM, mx), (L.DIAG_YMOM, my), (L.DIAG_ZMOM, mz), (L.DIAG_RHO_E_INT, eint),
                 (L.DIAG_RHO_E, eden), (L.DIAG_SPECIES, rx)):
        terms[m], unit[m] = t, 2.0 ** -23
    for m, t in ((L.DIAG_ANGMOM_X, (Y - 256) * mz - (Z - 256) * my), (L.DIAG_ANGMOM_Y, (Z - 256) * mx - (X - 256) * mz),
                 (L.DIAG_ANGMOM_Z, (X - 256) * my - (Y - 256) * mx), (L.DIAG_COM_X, rho * X), (L.DIAG_COM_Y, rho * Y),
                 (L.DIAG_COM_Z, rho * Z)):
        terms[m], unit[m] = t + np.zeros(shape, dtype=np.int64), 2.0 ** -32
    terms[L.DIAG_RHO_K], unit[L.DIAG_RHO_K] = (4 // rho) * (mx * mx + my * my + mz * mz), 2.0 ** -26      # 0.5 / rho in eighths
    # the same terms as diag_add forms them, in float64
    vol = 2.0 ** -23
    x0, x1, x2 = X * 2.0 ** -9, Y * 2.0 ** -9, Z * 2.0 ** -9
    l0, l1, l2 = x0 - 0.5, x1 - 0.5, x2 - 0.5
    fr, fx, fy, fz = (S[m].astype(np.float64) for m in (0, 1, 2, 3))
    fterms = {L.DIAG_MASS: fr * vol, L.DIAG_XMOM: fx * vol, L.DIAG_YMOM: fy * vol, L.DIAG_ZMOM: fz * vol,
              L.DIAG_ANGMOM_X: (l1 * fz - l2 * fy) * vol, L.DIAG_ANGMOM_Y: (l2 * fx - l0 * fz) * vol,
              L.DIAG_ANGMOM_Z: (l0 * fy - l1 * fx) * vol, L.DIAG_RHO_E_INT: S[5] * vol,
              L.DIAG_RHO_K: (0.5 / fr * (fx * fx + fy * fy + fz * fz)) * vol, L.DIAG_RHO_E: S[4] * vol,
              L.DIAG_COM_X: (fr * x0) * vol, L.DIAG_COM_Y: (fr * x1) * vol, L.DIAG_COM_Z: (fr * x2) * vol, L.DIAG_SPECIES: S[7] * vol}
    sums = {}
    for name, ki, kf in (("all", 1, 1.0), ("masked", mask.astype(np.int64), mask.astype(np.float64))):
        isum = np.array([int((terms[m] * ki).sum()) for m in range(14)], dtype=np.int64)
        assert np.all(np.abs(isum) < 2 ** 52) and np.all(isum != 0)
        want = isum.astype(np.float64) * unit
        # the exactness condition: float64 sums of the float64 terms, in numpy's order, are the integer sums
        fsum = np.array([np.sum(fterms[m] * kf) for m in range(14)])
        assert np.array_equal(_bits(fsum), _bits(want)), (name, fsum, want)
        sums[name] = want
    _CACHE["diag"] = (S, mask, sums)
    return _CACHE["diag"]


def test_integrated_quantities_with_doubled_iters(hydro):
    """255 x 128 x 130 zones in a FAB of 4 NaN ghost zones, rows on an odd zone: 2 129 920 pairs, more than 2048 workgroups take at
    four pairs a thread, so `iters` = 8.  The sums are exact in any order: bit equality in both builds, unmasked and masked."""
    from castro_amd import _lib
    c = G.DIAG_LARGE
    lo, ext, ng = c["lo"], c["ext"], c["ng"]
    hi = tuple(lo[d] + ext[d] - 1 for d in range(3))
    S, mask, sums = _diag_state()
    geom = _lib.make_geom(c["n_cell"])
    assert tuple(geom.dx[d] for d in range(3)) == (2.0 ** -8, 2.0 ** -7, 2.0 ** -8)
    F = torch.full((8, ext[2] + 2 * ng, ext[1] + 2 * ng, ext[0] + 2 * ng), NAN, dtype=torch.float64, device="cuda")
    valid = F[:, ng:-ng, ng:-ng, ng:-ng]
    valid.copy_(torch.from_numpy(S).cuda())
    fbox = (tuple(x - ng for x in lo), tuple(x + ng for x in hi))

    def run(m):
        boxes = hydro.make_diag_boxes([(lo, hi, (F, fbox), m)])
        out = torch.full((14,), NAN, dtype=torch.float64, device="cuda")
        hydro.integrated_quantities_mf(boxes, geom, (0.5, 0.5, 0.5), out)
        torch.cuda.synchronize()
        return out.cpu().numpy(), hydro.diag_workgroups(boxes)

    got, nb = run(None)
    pairs = G.diag_pairs()
    assert nb * 256 * 4 < pairs <= nb * 256 * 8, "more than four pairs a thread: iters = 8"
    assert np.array_equal(_bits(got), _bits(sums["all"])), (got, sums["all"])
    md = torch.from_numpy(mask).cuda()
    valid[:, md == 0] = NAN
    got, nb = run(md)
    assert nb * 256 * 4 < pairs
    assert np.array_equal(_bits(got), _bits(sums["masked"])), (got, sums["masked"])


# ---- 6. pack, min / max and unpack with iters = 8 and 16 ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one_zone", "vec2", "both"])
def test_pack_minmax_unpack_with_doubled_iters(hydro, which):
    """entries of 8 components with more than 524 288 items each: 4320 (one zone per access) and 4608 (two) workgroups at four
    items a thread, so each alone runs with `iters` = 8, both in one call with 16.  Ghost zones are NaN."""
    SENT = -12345.0
    ents = {"one_zone": [G.PACK_ONE_ZONE], "vec2": [G.PACK_VEC2], "both": [G.PACK_ONE_ZONE, G.PACK_VEC2]}[which]
    rng = np.random.default_rng(61)
    dev = []
    for e in ents:
        t, box, reg = _fab(rng, e["lo"], e["ext"], e["ncomp"], e["ng"], np.nan)
        dev.append((torch.from_numpy(t).cuda(), box, reg))
    entries = hydro.make_pack_entries(dev)
    _, n, doubles, pairs = entries
    assert pairs == 8 * len(ents) and doubles == sum(8 * G.zones(e["ext"]) for e in ents)

    def reference():
        flat = [_valid(*f).reshape(f[0].shape[0], -1) for f in dev]
        return torch.cat([x.reshape(-1) for x in flat]), torch.cat([x.amin(dim=1) for x in flat] + [x.amax(dim=1) for x in flat])

    def pack(minmax=True):
        dst = torch.full((doubles + 4,), 777.0, dtype=torch.float64, device="cuda")
        mm = torch.full((2 * pairs + 2,), 777.0, dtype=torch.float64, device="cuda") if minmax else None
        hydro.fab_pack(entries, dst, mm)
        torch.cuda.synchronize()
        assert bool((dst[doubles:] == 777.0).all()) and (mm is None or bool((mm[2 * pairs:] == 777.0).all()))
        return dst[:doubles], None if mm is None else mm[:2 * pairs]

    want, want_mm = reference()
    assert not bool(torch.isnan(want).any())
    buf, mm = pack()
    assert _eq(buf, want), "the buffer against torch slicing"
    assert _eq(mm, want_mm), "min / max against amin / amax per (entry, component)"
    assert _eq(pack(minmax=False)[0], want), "the copy alone"
    # unpack into sentinel-filled FABs: the valid zones come back, every ghost zone keeps its bits
    back = [(torch.full_like(t, SENT), box, reg) for t, box, reg in dev]
    hydro.fab_unpack(hydro.make_pack_entries(back), buf)
    torch.cuda.synchronize()
    sent = torch.tensor(SENT, dtype=torch.float64).view(torch.int64).item()
    for (t, box, reg), (u, _, _) in zip(dev, back):
        assert _eq(_valid(u, box, reg), _valid(t, box, reg))
        ghost = torch.ones_like(u, dtype=torch.bool)
        _valid(ghost, box, reg)[...] = False
        assert bool((u.view(torch.int64)[ghost] == sent).all()), "every ghost zone is left at the sentinel"
    del back
    # a NaN in the last valid zone of one component -- the last item of the last trip of its last workgroup
    pair = 8 * (len(ents) - 1) + 5
    _valid(*dev[-1])[5, -1, -1, -1] = NAN
    want, want_mm = reference()
    nan = torch.isnan(want_mm)
    assert nan.nonzero().flatten().tolist() == [pair, pairs + pair]
    buf, got_mm = pack()
    assert _eq(buf, want), "the copy carries the NaN with its bits"
    assert torch.equal(torch.isnan(got_mm), nan) and _eq(got_mm[~nan], mm[~nan]), "exactly that pair's minimum and maximum"

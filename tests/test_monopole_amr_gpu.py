"""GPU tests of monopole gravity on AMR levels (the new kernels of castro_amd/csrc/monopole_kernels.hip, the GravFab instantiation of
the one-pass source kernel, CastroAmr(gravity=MonopoleGravity(...))), for both numerics builds.  Reference and tolerances:
tests/monopole_amr_ref.py -- counts exactly, bin masses within N_bin 2^-52 A_bin, the combination and the boundary fill bit for
bit, interpolation and one-pass sources bit for bit in the `exact` build and within 1e-10 of the field's max in `contract`, the
driver within max(1e-10, 100 s) of the field's max."""
import os

import numpy as np
import pytest
import torch

from tests import monopole_amr_ref as A
from tests import monopole_ref as R
from tests.util import physical_state

pytestmark = pytest.mark.gpu

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


def _close(h, got, want, what):
    """`exact`: the same bits; `contract`: within 1e-10 of the largest magnitude of the field"""
    if h.numerics == "exact":
        assert np.array_equal(got, want), "%s: %d entries differ, max %g" % (what, int((got != want).sum()), np.abs(got - want).max())
    else:
        d, m = np.abs(got - want).max(), np.abs(want).max()
        print("%s (contract): max deviation %.3g of %.3g, bit-equal: %s" % (what, d, m, np.array_equal(got, want)))
        assert d <= 1e-10 * m, (what, d, m)


# ---- castro_amd_radial_mass_mf_ex ------------------------------------------------------------------------------------------------
EX_N, EX_HI = (28, 10, 8), (3.5, 1.25, 1.0)           # cubic zones of 0.125; the boxes 0..15 x 8 x 8 and 16..27 x 10 x 6


def _ex_boxes():
    """a 16 x 8 x 8 box and a 12 x 10 x 6 box (partial bricks, an odd row length in the FAB), old and new states on FABs with 2 and
    3 NaN ghost zones; the second box carries a mask with a hole and a few zones whose interpolated density is zero"""
    if "ex" not in _CACHE:
        rng = np.random.default_rng(5)
        out = []
        for lo, hi, ng in (((0, 0, 0), (15, 7, 7), 2), ((16, 0, 1), (27, 9, 6), 3)):
            ext = tuple(hi[d] - lo[d] + 1 for d in range(3))
            Uo, Un = physical_state(rng, lo, hi, jump=False), physical_state(rng, lo, hi, jump=False)
            mask = None
            if lo[0] == 16:
                mask = np.ones(ext[::-1], dtype=np.uint8)
                mask[1:4, 3:7, 2:9] = 0
                Uo[0][0, 0, :3] = 0.0
                Un[0][0, 0, :3] = 0.0
            fabs = []
            for U in (Uo, Un):
                F = np.full((8,) + tuple(e + 2 * ng for e in ext[::-1]), np.nan)
                F[:, ng:ng + ext[2], ng:ng + ext[1], ng:ng + ext[0]] = U
                fabs.append(F)
            fbox = (tuple(x - ng for x in lo), tuple(x + ng for x in hi))
            out.append((Uo[0].copy(), Un[0].copy(), lo, hi, mask, fabs, fbox))
        _CACHE["ex"] = out
    return _CACHE["ex"]


@pytest.mark.parametrize("drdxfac", [2, 4])
@pytest.mark.parametrize("weights", [(0.5, 0.5), (0.7, 0.3)])
def test_radial_mass_ex(hydro, drdxfac, weights):
    from castro_amd import _lib
    geom = _lib.make_geom(EX_N, prob_hi=EX_HI)
    mono = _lib.make_monopole(EX_N, geom, (0.0, 0.0, 0.0), drdxfac)
    boxes = _ex_boxes()
    oa, al = weights
    key = ("exref", drdxfac, weights)
    if key not in _CACHE:
        _CACHE[key] = A.radial_mass_ex([(ro, rn, lo, mask, oa, al) for ro, rn, lo, hi, mask, fabs, fbox in boxes], geom, mono)
    ref = _CACHE[key]
    assert ref["count"].sum() > 0
    dev = [(torch.from_numpy(b[5][0]).cuda(), torch.from_numpy(b[5][1]).cuda(), None if b[4] is None else torch.from_numpy(b[4]).cuda())
           for b in boxes]
    table = hydro.make_radial_boxes([(b[2], b[3], (d[0], b[6]), (d[1], b[6]), d[2]) for b, d in zip(boxes, dev)])

    def call(stream=None):
        out = torch.full((2 * mono.n1d,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        hydro.radial_mass_mf_ex(table, oa, al, geom, mono, out, stream=stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    got = call()
    mass, vol = got[:mono.n1d], got[mono.n1d:]
    vf = R.vol_frac(geom, mono)
    assert np.array_equal(np.rint(vol / vf).astype(np.int64), ref["count"]), "the counts are integers and equal the restatement's"
    assert np.array_equal(vol, ref["vol"])
    bound = R.mass_bounds(ref)
    err = np.abs(mass - ref["mass"])
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("radial mass ex drdxfac %d weights %s (%s): worst deviation / bound = %.3g" % (drdxfac, weights, hydro.numerics, worst))
    assert np.all(err <= bound)
    assert np.array_equal(call().view(np.int64), got.view(np.int64)), "two calls: the same bits"
    assert np.array_equal(call(stream=torch.cuda.Stream()).view(np.int64), got.view(np.int64)), "another stream: the same bits"
    # the single-state call on the same boxes is what weights (1, 0) would bin -- and differs from the interpolated one
    one = torch.empty(2 * mono.n1d, dtype=torch.float64, device="cuda")
    hydro.radial_mass_mf(hydro.make_diag_boxes([(b[2], b[3], (d[0], b[6]), d[2]) for b, d in zip(boxes, dev)]), geom, mono, one)
    assert not np.array_equal(one.cpu().numpy()[:mono.n1d], mass)


# ---- castro_amd_radial_combine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [2, 3])
def test_radial_combine(hydro, levels):
    from castro_amd import _lib
    base, drdxfac = (24, 20, 16), 2
    n1ds = [_lib.monopole_n1d(tuple((2 ** l) * x for x in base), drdxfac) for l in range(levels)]
    assert n1ds[-1] != 2 ** (levels - 1) * n1ds[0], "n1d of a level is no exact multiple of the coarser one"
    rng = np.random.default_rng(3)
    arrs = [(rng.uniform(0.5, 2.0, n) * 10.0 ** rng.integers(-3, 4, n), rng.uniform(0.0, 1.0, n)) for n in n1ds]
    level = levels - 1
    wm, wv = A.combine(arrs, n1ds, level)
    dev = [torch.from_numpy(np.concatenate(a)).cuda() for a in arrs]
    out = torch.full((2 * n1ds[level],), float("nan"), dtype=torch.float64, device="cuda")
    hydro.radial_combine(level, dev, n1ds, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n1ds[level]].view(np.int64), wm.view(np.int64))
    assert np.array_equal(got[n1ds[level]:].view(np.int64), wv.view(np.int64))
    # a coarser array shorter than n1d / ratio is refused
    short = list(n1ds)
    short[0] = n1ds[level] // 2 ** level - 1
    with pytest.raises(RuntimeError):
        hydro.radial_combine(level, dev, short, out)


# ---- the Gravity_Type ghost zones: boundary fill and coarse-fine interpolation ---------------------------------------------------
def test_grav_bc_fill(hydro):
    """a 12 x 10 x 6 domain with symmetry (x lo), outflow (x hi, y hi), wall (y lo, z lo, z hi) faces, the FAB grown by one"""
    from castro_amd import _lib
    n = (12, 10, 6)
    geom = _lib.make_geom(n, lo_bc=(3, 4, 5), hi_bc=(2, 2, 4))
    box = ((-1, -1, -1), (12, 10, 6))
    rng = np.random.default_rng(9)
    g = rng.normal(size=(3, 8, 12, 14))
    want = g.copy()
    outside = A.grav_bc_fill(want, box, geom)
    assert outside.sum() == 14 * 12 * 8 - 12 * 10 * 6
    assert np.array_equal(want[0][1:-1, 1:-1, 0], -g[0][1:-1, 1:-1, 1]) and np.array_equal(want[1][1:-1, 1:-1, 0], g[1][1:-1, 1:-1, 1])
    t = torch.from_numpy(g).cuda()
    hydro.grav_bc_fill(t, box, geom)
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), "no arithmetic beyond a sign: the same bits in both builds"
    # a box in the corner of a larger domain: only the zones outside the domain change
    geom2 = _lib.make_geom((24, 20, 12), lo_bc=(3, 4, 5), hi_bc=(2, 2, 4))
    want2 = g.copy()
    A.grav_bc_fill(want2, box, geom2)
    t2 = torch.from_numpy(g).cuda()
    hydro.grav_bc_fill(t2, box, geom2)
    assert np.array_equal(t2.cpu().numpy().view(np.int64), want2.view(np.int64))
    assert np.array_equal(want2[:, 1:, 1:, 1:], g[:, 1:, 1:, 1:])


def test_grav_coarse_fine_ghosts(hydro, oracle):
    """the ghost shell of a 12 x 10 x 6 fine gravity FAB from coarse grav_old / grav_new, interpolated in time (lincomb) and space
    (CASTRO_AMD_OP_INTERP with 3 components), against the CPU backend's lincomb + cc_interp"""
    from castro_amd import _lib as L
    from castro_amd.castro import shell_slabs
    fbx = ((8, 6, 4), (19, 15, 9))
    gbox = (tuple(x - 1 for x in fbx[0]), tuple(x + 1 for x in fbx[1]))
    cbox = (tuple(x // 2 - 1 for x in gbox[0]), tuple(x // 2 + 1 for x in gbox[1]))
    rng = np.random.default_rng(21)
    shape_c = tuple(cbox[1][d] - cbox[0][d] + 1 for d in (2, 1, 0))
    co, cn = rng.normal(size=(3,) + shape_c), rng.normal(size=(3,) + shape_c)
    shape_f = tuple(gbox[1][d] - gbox[0][d] + 1 for d in (2, 1, 0))
    f0 = rng.normal(size=(3,) + shape_f)
    a = 0.5
    ob = A.MonopoleAmrOracleBackend()
    ctmp, want = torch.zeros((3,) + shape_c, dtype=torch.float64), torch.from_numpy(f0.copy())
    ob.lincomb(ctmp, cbox, 1.0 - a, torch.from_numpy(co), cbox, a, torch.from_numpy(cn), cbox, 3, cbox[0], cbox[1])
    slabs = [s for s in shell_slabs(gbox, fbx) if all(s[1][d] >= s[0][d] for d in range(3))]
    for lo, hi in slabs:
        ob.cc_interp(ctmp, cbox, want, gbox, lo, hi, 3)
    dco, dcn, dct, df = (torch.from_numpy(x).cuda() for x in (co, cn, np.zeros((3,) + shape_c), f0))
    ops = hydro.make_ops([(L.OP_LINCOMB, 0, 3, cbox[0], cbox[1], 1.0 - a, a, (dct, cbox), (dco, cbox), (dcn, cbox))])
    hydro.fab_ops(ops, params=L.default_params())
    hydro.fab_ops(hydro.make_ops([(L.OP_INTERP, 0, 3, lo, hi, 0.0, 0.0, (df, gbox), (dct, cbox), None) for lo, hi in slabs]),
                  params=L.default_params())
    torch.cuda.synchronize()
    got = df.cpu().numpy()
    _close(hydro, got, want.numpy(), "gravity ghost shell")
    assert np.array_equal(got[:, 1:-1, 1:-1, 1:-1], f0[:, 1:-1, 1:-1, 1:-1]), "the valid zones are not touched"


# ---- castro_amd_sources_mf_g -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gtype", [1, 2, 3, 4])
def test_one_pass_sources_with_gravity_fabs(hydro, gtype):
    """two unequal boxes: the one-pass kernel on the GravFab accessor against zero + the _gfab source call + apply_source, both on
    the device"""
    from castro_amd import _lib as L
    P = L.default_params()
    geom = L.make_geom((28, 10, 8), prob_hi=(3.5, 1.25, 1.0))
    rng = np.random.default_rng(17 + gtype)
    dt = 1.e-3
    boxes = []
    for lo, hi in (((0, 0, 0), (15, 7, 7)), ((16, 0, 1), (27, 9, 6))):
        gb = (tuple(x - 4 for x in lo), tuple(x + 4 for x in hi))
        vb = (tuple(x - 1 for x in lo), tuple(x + 1 for x in hi))
        sb = (tuple(x - 3 for x in lo), tuple(x + 3 for x in hi))
        So, Sn = (torch.from_numpy(physical_state(rng, gb[0], gb[1], jump=False)).cuda() for _ in range(2))
        shp = lambda b: tuple(b[1][d] - b[0][d] + 1 for d in (2, 1, 0))
        go, gn = (torch.from_numpy(rng.normal(size=(3,) + shp(vb))).cuda() for _ in range(2))
        fb, mf = [], []
        for d in range(3):
            fhi = list(hi); fhi[d] += 1
            fb.append((lo, tuple(fhi)))
            mf.append(torch.from_numpy(rng.normal(size=(1,) + shp((lo, tuple(fhi))))).cuda())
        boxes.append(dict(lo=lo, hi=hi, gb=gb, vb=vb, sb=sb, So=So, Sn=Sn, go=go, gn=gn, fb=fb, mf=mf))
    for stage in (0, 1):
        want, got = [], []
        for b in boxes:
            sbx = b["sb"] if stage == 0 else (b["lo"], b["hi"])
            shp = tuple(sbx[1][d] - sbx[0][d] + 1 for d in (2, 1, 0))
            # the separate calls
            src = torch.zeros((7,) + shp, dtype=torch.float64, device="cuda")
            Sn = b["Sn"].clone()
            if stage == 0:
                hydro.old_gravity_source_gfab(b["So"], b["gb"], src, sbx, b["lo"], b["hi"], b["go"], b["vb"], gtype, dt)
            else:
                hydro.new_gravity_source_gfab(b["So"], b["gb"], Sn, b["gb"], src, sbx, b["mf"], b["fb"], b["lo"], b["hi"], b["go"], b["gn"],
                                              b["vb"], gtype, dt, geom)
            hydro.apply_source(Sn, b["gb"], b["So"] if stage == 0 else Sn, b["gb"], dt, src, sbx, 7, b["lo"], b["hi"], P, ntimes=1)
            want.append((src, Sn))
            got.append((torch.full((7,) + shp, float("nan"), dtype=torch.float64, device="cuda"), b["Sn"].clone(), sbx))
        table = hydro.make_source_boxes([(b["lo"], b["hi"], (b["So"], b["gb"]), (g[1], b["gb"]), (g[0], g[2]), b["mf"], b["fb"])
                                         for b, g in zip(boxes, got)])
        gold = hydro.make_grav_fabs([(b["go"], b["vb"]) for b in boxes])
        gnew = hydro.make_grav_fabs([(b["gn"], b["vb"]) for b in boxes])
        hydro.sources_mf_g(stage, table, gold, gnew, gtype, None, geom, P, dt, ntimes=1)
        torch.cuda.synchronize()
        for n, (b, w, g) in enumerate(zip(boxes, want, got)):
            lo, hi, gbx = b["lo"], b["hi"], b["gb"]
            vs = (slice(None),) + tuple(slice(lo[d] - gbx[0][d], hi[d] - gbx[0][d] + 1) for d in (2, 1, 0))
            _close(hydro, g[0].cpu().numpy(), w[0].cpu().numpy(), "stage %d type %d box %d source" % (stage, gtype, n))
            _close(hydro, g[1].cpu().numpy()[vs], w[1].cpu().numpy()[vs], "stage %d type %d box %d state" % (stage, gtype, n))
            assert np.abs(w[0].cpu().numpy()).max() > 0.0


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def _reference(oracle):
    if "amr" not in _CACHE:
        ref, dts, s = A.dust_amr_sensitivity(oracle)
        _CACHE["amr"] = (A.level_states(ref), dts, s, [ref.gravity.radial_gravity(l) for l in range(len(ref.lev))])
    return _CACHE["amr"]


def _device_run(numerics):
    import castro_amd
    from castro_amd import _lib
    a, dts = A.dust_amr_run(lambda: castro_amd.HipHydro(0, numerics=numerics), _lib.default_params(**R.DUST_PARAMS))
    torch.cuda.synchronize()
    return a, dts


def test_dust_collapse_amr_driver_against_the_restatement(hydro, oracle):
    """The dust collapse on base 16^3 + a fixed 16^3 fine patch, drdxfac 2, 2 coarse steps (four fine advances: old, interpolated
    and new coarse data), against the same driver on MonopoleAmrOracleBackend.  Not bitwise: the bin sums differ in order.
    Tolerance per field and level: max(1e-10, 100 s) of the field's max, s the deviation the CPU backend shows between two runs
    whose radial masses differ by one ulp per bin (measured on the reference side, printed)."""
    want, dts, s, rg = _reference(oracle)
    a, gdts = _device_run(hydro.numerics)
    assert np.allclose(np.array(gdts), np.array(dts), rtol=1e-12, atol=0.0), (gdts, dts)
    for l, (w, got) in enumerate(zip(want, A.level_states(a))):
        tol = np.maximum(1e-10, 100.0 * s[l])
        d = R.field_deviation(got, w)
        print("AMR dust collapse (%s) level %d: s" % (hydro.numerics, l), s[l], "deviation", d, "tolerance", tol)
        assert np.all(d <= tol), (l, d, tol)
        m, v, go, gn = a.gravity.radial_gravity(l)
        assert np.array_equal(v, rg[l][1]), "the volumes of level %d are equal" % l
        assert np.abs(gn - rg[l][3]).max() <= 1e-9 * np.abs(rg[l][3]).max()
        assert np.all(gn[1:a.gravity.n1d(l) // 3] < 0.0), "gravity points inwards"


def test_one_pass_and_separate_calls_agree(hydro):
    """the same run with the gravity sources inside the one-pass kernel and as separate calls: the same bits in `exact`, the
    1e-10 bar in `contract`"""
    if ("dev", hydro.numerics) not in _CACHE:
        _CACHE[("dev", hydro.numerics)] = A.level_states(_device_run(hydro.numerics)[0])
    one = _CACHE[("dev", hydro.numerics)]
    os.environ["CASTRO_AMD_SOURCES_ONE_PASS"] = "0"
    try:
        sep = A.level_states(_device_run(hydro.numerics)[0])
    finally:
        del os.environ["CASTRO_AMD_SOURCES_ONE_PASS"]
    for l, (x, y) in enumerate(zip(one, sep)):
        _close(hydro, x, y, "one-pass against separate calls, level %d" % l)


def test_single_level_and_level_zero_are_one_route(hydro):
    """grav_source_type = 2 reads no ghost zone of the field: Castro(gravity_type="monopole") and a CastroAmr with no refined
    level agree bit for bit after two steps, in either build"""
    import castro_amd
    from castro_amd import _lib
    c, a = A.single_and_hierarchy(lambda: castro_amd.HipHydro(0, numerics=hydro.numerics), _lib.default_params(**R.DUST_PARAMS),
                                  grav_source_type=2)
    torch.cuda.synchronize()
    A.assert_routes_agree_inside(c, a)

"""GPU tests of monopole self-gravity (castro_amd/csrc/monopole_kernels.hip, the _gfab gravity sources of aux_kernels.hip and
Castro(gravity_type="monopole")), for both numerics builds.  Reference and tolerances: tests/monopole_ref.py -- bins and
counts exactly, bin masses within N_bin 2^-52 A_bin, the integration bit for bit, interpolation and sources bit for bit in the
`exact` build and within 1e-10 of the field's max in `contract`, the driver within max(1e-10, 100 s) of the field's max."""
import numpy as np
import pytest
import torch

from tests import monopole_ref as R
from tests.util import physical_state

pytestmark = pytest.mark.gpu

N_CELL = (24, 20, 16)
PROB_HI = (3.0, 2.5, 2.0)                 # cubic zones of 0.125
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


def _geom():
    from castro_amd import _lib
    return _lib.make_geom(N_CELL, prob_hi=PROB_HI)


def _close(h, got, want, what):
    """`exact`: the same bits; `contract`: within 1e-10 of the largest magnitude of the field"""
    if h.numerics == "exact":
        assert np.array_equal(got, want), "%s: %d entries differ, max %g" % (what, int((got != want).sum()), np.abs(got - want).max())
    else:
        d, m = np.abs(got - want).max(), np.abs(want).max()
        print("%s (contract): max deviation %.3g of %.3g" % (what, d, m))
        assert d <= 1e-10 * m, (what, d, m)


# ---- binning ---------------------------------------------------------------------------------------------------------------------
def _bin_boxes():
    """the domain as three unequal boxes cut at odd x (0..6 | 7..17 | 18..23), on FABs with 1, 4 and 3 NaN ghost zones (the
    valid zones of the first and the last start at an odd distance from a 16-byte boundary); a mask with scattered zeros on
    the second, a few zones of zero density in the third"""
    if "boxes" not in _CACHE:
        rng = np.random.default_rng(11)
        out = []
        for (x0, x1), ng in (((0, 6), 1), ((7, 17), 4), ((18, 23), 3)):
            lo, hi = (x0, 0, 0), (x1, N_CELL[1] - 1, N_CELL[2] - 1)
            ext = tuple(hi[d] - lo[d] + 1 for d in range(3))
            U = physical_state(rng, lo, hi, jump=False)
            mask = None
            if x0 == 7:
                mask = (rng.uniform(size=ext[::-1]) > 0.15).astype(np.uint8)
            if x0 == 18:
                U[0][rng.uniform(size=ext[::-1]) < 0.05] = 0.0
            F = np.full((8,) + tuple(e + 2 * ng for e in ext[::-1]), np.nan)
            F[:, ng:ng + ext[2], ng:ng + ext[1], ng:ng + ext[0]] = U
            fbox = (tuple(x - ng for x in lo), tuple(x + ng for x in hi))
            out.append((U[0].copy(), lo, hi, mask, F, fbox))
        _CACHE["boxes"] = out
    return _CACHE["boxes"]


BIN_CASES = [(1, "mid", None), (2, "mid", None), (4, "mid", None), (1, "lo", None), (2, "lo", None), (4, "lo", None),
             (4, "mid", 40), (2, "lo", 33)]


@pytest.mark.parametrize("drdxfac,where,n1d", BIN_CASES)
def test_radial_mass(hydro, drdxfac, where, n1d):
    from castro_amd import _lib
    geom = _geom()
    center = (1.5, 1.25, 1.0) if where == "mid" else (0.0, 0.0, 0.0)
    mono = _lib.make_monopole(N_CELL, geom, center, drdxfac, n1d=n1d)
    boxes = _bin_boxes()
    key = ("ref", drdxfac, where, n1d)
    if key not in _CACHE:
        _CACHE[key] = R.radial_mass([(rho, lo, mask) for rho, lo, hi, mask, F, fbox in boxes], geom, mono)
    ref = _CACHE[key]
    assert R.octant_factor(geom, mono) == (8.0 if where == "lo" else 1.0)
    assert (ref["dropped"] > 0) == (n1d is not None), "a short n1d drops sub-zones, the domain's own n1d none"
    dev = [(torch.from_numpy(F).cuda(), None if mask is None else torch.from_numpy(mask).cuda()) for _, _, _, mask, F, _ in boxes]
    table = hydro.make_diag_boxes([(b[1], b[2], (d[0], b[5]), d[1]) for b, d in zip(boxes, dev)])

    def call(stream=None):
        out = torch.full((2 * mono.n1d,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        hydro.radial_mass_mf(table, geom, mono, out, stream=stream)
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
    print("radial mass drdxfac %d centre %s n1d %d (%s): worst deviation / bound = %.3g" % (drdxfac, where, mono.n1d, hydro.numerics, worst))
    assert np.all(err <= bound)
    assert np.all(mass[ref["count"] == 0] == 0.0)
    again = call()
    assert np.array_equal(again.view(np.int64), got.view(np.int64)), "two calls: the same bits"
    other = call(stream=torch.cuda.Stream())
    assert np.array_equal(other.view(np.int64), got.view(np.int64)), "another stream: the same bits"


def test_radial_mass_refuses_a_drdxfac_beyond_the_window(hydro):
    from castro_amd import _lib
    geom = _geom()
    mono = _lib.make_monopole(N_CELL, geom, (1.5, 1.25, 1.0), 6)
    b = _bin_boxes()[0]
    table = hydro.make_diag_boxes([(b[1], b[2], (torch.from_numpy(b[4]).cuda(), b[5]), None)])
    out = torch.zeros(2 * mono.n1d, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        hydro.radial_mass_mf(table, geom, mono, out)


# ---- integration -----------------------------------------------------------------------------------------------------------------
def test_radial_gravity_is_the_restatement_bit_for_bit(hydro):
    from castro_amd import _lib
    geom = _geom()
    n1d = 37
    mono = _lib.make_monopole(N_CELL, geom, (1.5, 1.25, 1.0), 2, n1d=n1d)
    dr = geom.dx[0] / 2.0
    mono.max_radius_all_in_domain = 18.3 * dr            # mid-array: bins 0..17 take the second branch, 18.. the third
    rng = np.random.default_rng(3)
    mass = rng.uniform(0.0, 5.0, size=n1d)
    vol = rng.uniform(0.1, 2.0, size=n1d)
    empty = rng.uniform(size=n1d) < 0.2
    empty[[5, 20, 36]] = True
    mass[empty], vol[empty] = 0.0, 0.0
    mv = torch.from_numpy(np.concatenate([mass, vol])).cuda()
    out = torch.full((n1d,), float("nan"), dtype=torch.float64, device="cuda")
    hydro.radial_gravity(mono, geom, mv, out)
    torch.cuda.synchronize()
    want = R.radial_gravity(mass, vol, geom, mono)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), np.abs(got - want).max()


# ---- interpolation ---------------------------------------------------------------------------------------------------------------
def test_monopole_grav_interpolation(hydro):
    from castro_amd import _lib
    geom = _geom()
    n1d = 6
    mono = _lib.make_monopole(N_CELL, geom, (0.44, 0.41, 0.3), 1, n1d=n1d)
    rg = np.array([-1.0, -5.0, -1.2, -6.0, -0.5, -7.0])          # curvature of both signs: both clamps bite
    box = ((-1, -1, -1), (10, 8, 6))                             # a grown 12 x 10 x 8 FAB
    SENT = 12345.0
    want = np.full((3, 8, 10, 12), SENT)
    info = {}
    index = R.interpolate(rg, geom, mono, want, box, info)
    assert (index == 0).any() and (index == n1d - 1).any() and ((index > 0) & (index < n1d - 1)).any() and (index > n1d - 1).any()
    assert (info["clamp"] == -1).any() and (info["clamp"] == 1).any()
    G = torch.full((3, 8, 10, 12), SENT, dtype=torch.float64, device="cuda")
    hydro.monopole_grav(torch.from_numpy(rg).cuda(), mono, geom, G, box)
    torch.cuda.synchronize()
    got = G.cpu().numpy()
    beyond = index > n1d - 1
    assert np.all(got[:, beyond] == SENT) and np.all(got[:, ~beyond] != SENT)
    if hydro.numerics == "exact":
        assert np.array_equal(got, want)
    else:
        assert np.abs(got - want)[:, ~beyond].max() <= 1e-10 * np.abs(rg).max()


# ---- sources ---------------------------------------------------------------------------------------------------------------------
def _source_case():
    if "src" not in _CACHE:
        rng = np.random.default_rng(21)
        lo, hi = (3, 2, 1), (14, 11, 8)                          # 12 x 10 x 8
        gb = (tuple(x - 4 for x in lo), tuple(x + 4 for x in hi))
        sb = (tuple(x - 3 for x in lo), tuple(x + 3 for x in hi))
        vb = (tuple(x - 1 for x in lo), tuple(x + 1 for x in hi))
        UO = physical_state(rng, gb[0], gb[1], jump=True)
        UN = physical_state(rng, gb[0], gb[1], jump=True)
        fb, M = [], []
        for d in range(3):
            fhi = list(hi)
            fhi[d] += 1
            fb.append((lo, tuple(fhi)))
            M.append(rng.normal(size=(1,) + tuple(fhi[a] - lo[a] + 1 for a in (2, 1, 0))))
        shp = tuple(vb[1][a] - vb[0][a] + 1 for a in (2, 1, 0))
        z, y, x = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in shp], indexing="ij")
        a = rng.uniform(-1.0, 1.0, size=(2, 3, 4))
        g = [np.stack([a[t, n, 0] + a[t, n, 1] * np.sin(2.0 * x + n) + a[t, n, 2] * np.cos(3.0 * y) + a[t, n, 3] * z * x for n in range(3)])
             for t in range(2)]
        _CACHE["src"] = dict(lo=lo, hi=hi, gb=gb, sb=sb, vb=vb, UO=UO, UN=UN, fb=fb, M=M, gold=g[0], gnew=g[1],
                             sshape=(7,) + tuple(sb[1][a] - sb[0][a] + 1 for a in (2, 1, 0)))
    return _CACHE["src"]


def _gfab_sources(h, c, gold, gnew, gtype, dt, geom):
    """(old-time source, new-time source) of the _gfab calls, accumulated into zeroed Source_Type FABs, as numpy"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    UO, UN, go, gn, M = t(c["UO"]), t(c["UN"]), t(gold), t(gnew), [t(m) for m in c["M"]]
    so = torch.zeros(c["sshape"], dtype=torch.float64, device="cuda")
    sn = torch.zeros(c["sshape"], dtype=torch.float64, device="cuda")
    h.old_gravity_source_gfab(UO, c["gb"], so, c["sb"], c["lo"], c["hi"], go, c["vb"], gtype, dt)
    h.new_gravity_source_gfab(UO, c["gb"], UN, c["gb"], sn, c["sb"], M, c["fb"], c["lo"], c["hi"], go, gn, c["vb"], gtype, dt, geom)
    torch.cuda.synchronize()
    return so.cpu().numpy(), sn.cpu().numpy()


@pytest.mark.parametrize("gtype", [1, 2, 3, 4])
def test_gfab_sources_with_one_vector_equal_the_constant_gravity_calls(hydro, gtype):
    c, geom, dt = _source_case(), _geom(), 0.013
    vec = (0.3, -0.7, -9.8)
    g = np.empty_like(c["gold"])
    for n in range(3):
        g[n] = vec[n]
    so, sn = _gfab_sources(hydro, c, g, g, gtype, dt, geom)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    UO, UN, M = t(c["UO"]), t(c["UN"]), [t(m) for m in c["M"]]
    ro = torch.zeros(c["sshape"], dtype=torch.float64, device="cuda")
    rn = torch.zeros(c["sshape"], dtype=torch.float64, device="cuda")
    hydro.old_gravity_source(UO, c["gb"], ro, c["sb"], c["lo"], c["hi"], vec, gtype, dt)
    hydro.new_gravity_source(UO, c["gb"], UN, c["gb"], rn, c["sb"], M, c["fb"], c["lo"], c["hi"], vec, gtype, dt, geom)
    torch.cuda.synchronize()
    for n in range(7):
        for got, want, what in ((so, ro.cpu().numpy(), "old"), (sn, rn.cpu().numpy(), "new")):
            if np.abs(want[n]).max() == 0.0:
                assert np.all(got[n] == 0.0)
            else:
                _close(hydro, got[n], want[n], "%s source, component %d, type %d, one vector" % (what, n, gtype))


@pytest.mark.parametrize("gtype", [1, 2, 3, 4])
def test_gfab_sources_with_a_varying_vector_equal_the_restatement(hydro, gtype):
    c, geom, dt = _source_case(), _geom(), 0.013
    so, sn = _gfab_sources(hydro, c, c["gold"], c["gnew"], gtype, dt, geom)
    dx = [geom.dx[d] for d in range(3)]
    wo = R.old_gravity_source(c["UO"], c["gb"], c["gold"], c["vb"], c["lo"], c["hi"], gtype, dt)
    wn = R.new_gravity_source(c["UO"], c["gb"], c["UN"], c["gb"], c["M"], c["fb"], c["gold"], c["gnew"], c["vb"], c["lo"], c["hi"],
                              gtype, dt, dx)
    v = (slice(None),) + R._sl(c["sb"], c["lo"], c["hi"])
    outside = np.ones(c["sshape"], dtype=bool)
    outside[v] = False
    assert np.all(so[outside] == 0.0) and np.all(sn[outside] == 0.0), "only [lo, hi] is written"
    for n in range(7):
        for got, want, what in ((so[v], wo, "old"), (sn[v], wn, "new")):
            if np.abs(want[n]).max() == 0.0:
                assert np.all(got[n] == 0.0)
            else:
                _close(hydro, got[n], want[n], "%s source, component %d, type %d" % (what, n, gtype))


# ---- driver ----------------------------------------------------------------------------------------------------------------------
def test_dust_collapse_driver_against_the_restatement(hydro, oracle):
    """Dust collapse, 16^3 octant, drdxfac 4, 3 steps, against the same driver on MonopoleOracleBackend.  Not bitwise: the bin
    sums differ in order.  Tolerance per field: max(1e-10, 100 s) of the field's max, s the deviation the CPU backend shows
    between two runs whose radial masses differ by one ulp per bin (printed)."""
    from castro_amd import _lib
    if "dust" not in _CACHE:
        ref, dts, s = R.dust_sensitivity(oracle)
        free, _ = R.dust_collapse_run(R.MonopoleOracleBackend(), oracle.default_params(**R.DUST_PARAMS), do_grav=False)
        _CACHE["dust"] = (ref.S_new().numpy().copy(), dts, s, free.S_new().numpy().copy(), ref.radial_gravity())
    want, dts, s, free, (rm, rv, rgv) = _CACHE["dust"]
    print("dust collapse: s per field =", s)
    tol = np.maximum(1e-10, 100.0 * s)
    c, gdts = R.dust_collapse_run(hydro, _lib.default_params(**R.DUST_PARAMS))
    torch.cuda.synchronize()
    got = c.S_new().cpu().numpy()
    d = R.field_deviation(got, want)
    print("dust collapse (%s): deviation per field" % hydro.numerics, d, "tolerance", tol)
    assert np.all(d <= tol), (d, tol)
    assert np.allclose(np.array(gdts), np.array(dts), rtol=1e-12, atol=0.0), (gdts, dts)
    dfree = R.field_deviation(got, free)
    assert dfree[R.UMX] > 1e4 * tol[R.UMX], (dfree, tol)
    mass, vol, grav = c.radial_gravity()
    assert np.array_equal(vol, rv)
    assert np.abs(grav - rgv).max() <= 1e-9 * np.abs(rgv).max()
    rc = (np.arange(c.n1d) + 0.5) * (c.geom.dx[0] / R.DUST_DRDXFAC)
    inside = rc < 0.9 * R.DUST_PROB["r_0"]
    assert np.all(grav[inside] < 0.0) and np.all(np.diff(grav[inside]) < 0.0)


def test_out_of_domain_ghost_zone_keeps_the_interpolation(hydro):
    """grav_source_type = 4 reads the ghost zone of grav_new: on a single level it holds the interpolated value"""
    from castro_amd import _lib
    from tests import monopole_amr_ref as A
    c, _ = R.dust_collapse_run(hydro, _lib.default_params(**R.DUST_PARAMS), steps=1)
    torch.cuda.synchronize()
    assert c.grav_source_type == 4
    A.assert_ghost_zone_is_the_interpolation(c, exact=hydro.numerics == "exact")

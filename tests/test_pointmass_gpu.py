"""GPU tests of the central point mass (castro_amd/csrc/pointmass_kernels.hip, Castro(use_point_mass=True),
CastroAmr(use_point_mass=True)), for both numerics builds.  Reference: tests/pointmass_ref.py.

Tolerances.  k_add_pointmass: `exact` the bits of the restatement on every zone, ghost zones included; `contract`
1e-10 * (|value before| + |point-mass term|) per component.  The mass change: n 2^-52 sum |vol drho| with n <= 64 terms, the
bound of any summation order; the restore and the sign test bit for bit.  Single-level drivers against the run on the CPU
restatement backend: bit for bit in `exact` where no sum whose order differs enters, 1e-10 of a field's maximum in `contract`
and in the accreting run (its point mass carries the mass sum, whose order differs between device and numpy, from step 2 on).
The AMR gravity FABs: max(1e-10, 100 s) of a field's maximum, s the deviation of a CPU hierarchy whose radial masses differ by
one ulp per bin (the convention of tests/test_monopole_amr_gpu.py: the order of the bin sums differs between device and numpy)."""
import numpy as np
import pytest
import torch

from tests import monopole_amr_ref as A
from tests import monopole_ref as R
from tests import pointmass_ref as PR

pytestmark = pytest.mark.gpu

_CACHE = {}
EPS = 2.0 ** -52


@pytest.fixture(scope="module", params=["exact", "contract"])
def hydro(request):
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=request.param)
    yield h
    h.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. k_add_pointmass ----------------------------------------------------------------------------------------------------------
CENTER, GC, MASS = (0.9137, 1.1713, 2.6291), 6.67428e-8, 3.0e9
# valid 20 x 12 x 8 at lo = (5, 8, 3) plus one ghost zone; two more FABs of other sizes (odd row lengths, one without ghost zones)
FABS = [((4, 7, 2), (25, 20, 11)), ((26, 7, 2), (32, 11, 20)), ((0, 0, 0), (2, 4, 0))]


def _add_geom():
    from castro_amd import _lib
    return _lib.make_geom((64, 48, 32), (-1.0, 0.5, 2.0), (2.2, 2.42, 4.0), (2, 2, 2), (2, 2, 2))        # dx = 0.05, 0.04, 0.0625


def _add_case():
    if "add" not in _CACHE:
        rng = np.random.default_rng(2031)
        geom = _add_geom()
        out = []
        for lo, hi in FABS:
            n = tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0))
            before = rng.normal(size=(3,) + n)
            term = PR.pointmass_term((lo, hi), geom, CENTER, GC, MASS)
            for d in range(3):                  # no zone centre on the centre in any direction
                x = geom.problo[d] + (np.arange(lo[d], hi[d] + 1) + 0.5) * geom.dx[d] - CENTER[d]
                assert np.abs(x).min() > 1e-3 * geom.dx[d]
            assert np.isfinite(term).all() and np.abs(term).max() > 0.1
            out.append((lo, hi, before, term, before + term))
        _CACHE["add"] = out
    return _CACHE["add"]


def _check_add(h, got, before, term, want, what):
    if h.numerics == "exact":
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), "%s: %d entries differ, max %g" % (
            what, int((got != want).sum()), np.abs(got - want).max())
    else:
        ratio = np.abs(got - want) / (1e-10 * (np.abs(before) + np.abs(term)))
        print("%s (contract): largest deviation / bound = %.3g, bit-equal: %s" % (what, ratio.max(), np.array_equal(got, want)))
        assert ratio.max() <= 1.0


def test_add_pointmass_fab_and_mf(hydro):
    from castro_amd import _lib
    geom, pm = _add_geom(), _lib.make_pointmass(CENTER, GC)
    mass = torch.tensor([MASS, -1.0], dtype=torch.float64, device="cuda")
    case = _add_case()
    singles = []
    for lo, hi, before, term, want in case:
        g = _t(before)
        hydro.add_pointmass(g, (lo, hi), pm, geom, mass)
        torch.cuda.synchronize()
        got = g.cpu().numpy()
        _check_add(hydro, got, before, term, want, "add_pointmass %s" % (lo,))
        singles.append(got)
    dev = [_t(c[2]) for c in case]
    hydro.add_pointmass_mf(hydro.make_grav_fabs([(g, (c[0], c[1])) for g, c in zip(dev, case)]), pm, geom, mass)
    torch.cuda.synchronize()
    for g, one in zip(dev, singles):
        assert np.array_equal(g.cpu().numpy().view(np.int64), one.view(np.int64)), "_mf gives the bits of the _fab calls"
    assert mass.cpu().tolist() == [MASS, -1.0]


def test_argument_checks(hydro):
    import castro_amd
    from castro_amd import _lib
    geom, pm = _add_geom(), _lib.make_pointmass(CENTER, GC)
    bad = _lib.Geom.from_buffer_copy(geom)
    bad.coord = 1
    lo, hi, before = _add_case()[0][:3]
    g = _t(before)
    mass = torch.tensor([MASS, 0.0], dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        hydro.add_pointmass(g, (lo, hi), pm, bad, mass)
    S = torch.ones((8, 10, 10, 10), dtype=torch.float64, device="cuda")
    box = ((-1, -1, -1), (8, 8, 8))
    tab = hydro.make_pointmass_boxes([((0, 0, 0), (7, 7, 7), (S, box), (S, box))])
    with pytest.raises(RuntimeError, match="unsupported"):
        hydro.pointmass_delta_mf(tab, pm, bad, mass[1:])
    with pytest.raises(RuntimeError, match="unsupported"):
        hydro.pointmass_apply_mf(tab, pm, bad, mass[1:], mass[:1])
    torch.cuda.synchronize()
    assert np.array_equal(g.cpu().numpy(), before) and mass.cpu().tolist() == [MASS, 0.0]
    with pytest.raises(ValueError, match="do_grav"):
        castro_amd.Castro((16, 16, 16), hydro=hydro, use_point_mass=True, point_mass=1.0)


# ---- 2. the mass change and the restore --------------------------------------------------------------------------------------------
def _cuts():
    """box lists of a 16^3 level: eight 8^3 boxes (the cube split over all of them), two boxes, four slabs of which two miss it"""
    eight = [((i, j, k), (i + 7, j + 7, k + 7)) for k in (0, 8) for j in (0, 8) for i in (0, 8)]
    two = [((0, 0, 0), (15, 7, 15)), ((0, 8, 0), (15, 15, 15))]
    slabs = [((i, 0, 0), (i + 3, 15, 15)) for i in (0, 4, 8, 12)]
    return dict(eight=eight, two=two, slabs=slabs)


def _level_geom():
    from castro_amd import _lib
    return _lib.make_geom((16, 16, 16), (0.0, 0.0, 0.0), (1.6, 0.8, 2.4), (2, 2, 2), (2, 2, 2))


def _level_states(sign):
    """S_old, S_new (8, 16, 16, 16) with random positive entries; sign: of the mass change of the cube (+1, -1, 0)"""
    key = ("level", sign)
    if key not in _CACHE:
        rng = np.random.default_rng(77)
        So, Sn = rng.uniform(0.5, 2.0, size=(8, 16, 16, 16)), rng.uniform(0.5, 2.0, size=(8, 16, 16, 16))
        c = (slice(6, 10),) * 3
        if sign > 0:
            Sn[(0,) + c] = So[(0,) + c] + rng.uniform(-0.1, 0.4, size=(4, 4, 4))
        elif sign < 0:
            Sn[(0,) + c] = So[(0,) + c] - rng.uniform(-0.1, 0.4, size=(4, 4, 4))
        else:
            Sn[(0,) + c] = So[(0,) + c]
        _CACHE[key] = (So, Sn)
    return _CACHE[key]


def _cut(S, boxes, ng=2):
    """one FAB per box with ng ghost zones that hold other numbers than the neighbour's valid zones"""
    out = []
    for lo, hi in boxes:
        n = tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0))
        F = np.full((8,) + tuple(x + 2 * ng for x in n), 7.25)
        F[:, ng:ng + n[0], ng:ng + n[1], ng:ng + n[2]] = S[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]
        out.append((F, (tuple(x - ng for x in lo), tuple(x + ng for x in hi))))
    return out


@pytest.mark.parametrize("cut", ["eight", "two", "slabs"])
@pytest.mark.parametrize("sign", [1, -1, 0])
def test_delta_and_apply(hydro, cut, sign):
    from castro_amd import _lib
    geom, ctr = _level_geom(), (0.8, 0.4, 1.2)
    pm = _lib.make_pointmass(ctr, GC)
    boxes = _cuts()[cut]
    So, Sn = _level_states(sign)
    fo, fn = _cut(So, boxes), _cut(Sn, boxes)
    ref_boxes = [(lo, hi, o[0], o[1], n[0], n[1]) for (lo, hi), o, n in zip(boxes, fo, fn)]
    terms = PR.delta_terms(ref_boxes, geom, ctr)
    assert terms.size == 64
    want = PR.delta(ref_boxes, geom, ctr)
    do, dn = [_t(f[0]) for f in fo], [_t(f[0]) for f in fn]
    tab = hydro.make_pointmass_boxes([(lo, hi, (a, o[1]), (b, n[1])) for (lo, hi), a, b, o, n in zip(boxes, do, dn, fo, fn)])
    buf = torch.tensor([MASS, float("nan")], dtype=torch.float64, device="cuda")

    def delta(stream=None):
        buf[1] = float("nan")
        torch.cuda.synchronize()
        hydro.pointmass_delta_mf(tab, pm, geom, buf[1:], stream=stream)
        torch.cuda.synchronize()
        return buf[1:].cpu().numpy().copy()

    got = delta()
    bound = 64 * EPS * np.abs(terms).sum()
    print("delta %s sign %d (%s): %.17g against %.17g, deviation / bound = %.3g" % (cut, sign, hydro.numerics, got[0], want,
                                                                                  abs(got[0] - want) / bound if bound else 0.0))
    assert abs(got[0] - want) <= bound
    assert (got[0] > 0.0) if sign > 0 else ((got[0] < 0.0) if sign < 0 else (got[0] == 0.0))
    assert np.array_equal(delta().view(np.int64), got.view(np.int64)), "two calls: the same bits"
    assert np.array_equal(delta(stream=torch.cuda.Stream()).view(np.int64), got.view(np.int64)), "another stream: the same bits"
    _CACHE.setdefault(("delta bits", hydro.numerics, sign), got[0])
    assert _CACHE[("delta bits", hydro.numerics, sign)] == got[0], "the same bits for every cut of the level"
    hydro.pointmass_apply_mf(tab, pm, geom, buf[1:], buf[:1])
    torch.cuda.synchronize()
    m = float(buf[0])
    expect = [f[0].copy() for f in fn]
    new_m = PR.apply([(lo, hi, o[0], o[1], e, n[1]) for (lo, hi), o, e, n in zip(boxes, fo, expect, fn)], geom, ctr, float(got[0]), MASS)
    assert m == new_m and (m == MASS + got[0] if sign > 0 else m == MASS)
    for d, e, o in zip(dn, expect, do):
        assert np.array_equal(d.cpu().numpy().view(np.int64), e.view(np.int64)), "the whole FAB of S_new, ghost zones included"
    for d, f in zip(do, fo):
        assert np.array_equal(d.cpu().numpy(), f[0]), "S_old is read only"
    if sign > 0:
        assert any(not np.array_equal(e, f[0]) for e, f in zip(expect, fn)), "the restore changed the cube"


# ---- 3. single-level drivers -------------------------------------------------------------------------------------------------------
def _params(mod, **kw):
    return mod.default_params(**dict(dict(init_shrink=1.0), **kw))


def _compare(h, got, want, gdts, dts, what, bits=True):
    d = R.field_deviation(got, want)
    print("%s (%s): deviation per field" % (what, h.numerics), d, "dt", gdts)
    if h.numerics == "exact" and bits:
        assert np.array_equal(got, want), "%s: %d entries differ, deviation per field %s" % (what, int((got != want).sum()), d)
        assert list(gdts) == list(dts)
    else:
        assert np.all(d <= 1e-10), d
        assert np.allclose(gdts, dts, rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("const_grav", [0.0, -0.75])
def test_constant_gravity_plus_point_mass_against_the_cpu_driver(hydro, oracle, const_grav):
    from castro_amd import _lib
    key = ("const", const_grav)
    if key not in _CACHE:
        P = _params(oracle)
        c, dts = PR.pointmass_run(PR.PointMassOracleBackend(), P, PR.radial_flow_state(P, v0=0.5), steps=3, const_grav=const_grav)
        f, _ = PR.pointmass_run(PR.PointMassOracleBackend(), _params(oracle), PR.radial_flow_state(P, v0=0.5), steps=3,
                                const_grav=const_grav, point_mass=0.0)
        _CACHE[key] = (c.S_new().numpy().copy(), dts, c.grav_new.numpy().copy(), f.S_new().numpy().copy())
    want, dts, gwant, free = _CACHE[key]
    P = _params(_lib)
    c, gdts = PR.pointmass_run(hydro, P, PR.radial_flow_state(P, v0=0.5), steps=3, const_grav=const_grav)
    torch.cuda.synchronize()
    assert c.grav_fab and not c.monopole and c.point_mass == PR.PM_M
    _compare(hydro, c.S_new().cpu().numpy(), want, gdts, dts, "const_grav %g + point mass" % const_grav)
    g = c.grav_new.cpu().numpy()
    if hydro.numerics == "exact":
        assert np.array_equal(g, gwant)
    else:
        assert np.abs(g - gwant).max() <= 1e-10 * np.abs(gwant).max()
    assert R.field_deviation(c.S_new().cpu().numpy(), free)[1] > 1e-6, "the point mass acts"


def test_monopole_plus_point_mass_leaves_the_radial_arrays_alone(hydro):
    """dust collapse on 16^3, the first gravity construction: the point mass is not binned, so radial_gravity() has the same bits
    with and without it, and the gravity FAB differs by the restated term"""
    import castro_amd
    from castro_amd import _lib
    M = 2.0e33
    out = []
    for pm in (False, True):
        c = castro_amd.Castro(R.DUST_N, params=_lib.default_params(**R.DUST_PARAMS), hydro=hydro, do_grav=True, gravity_type="monopole",
                              drdxfac=R.DUST_DRDXFAC, use_point_mass=pm, point_mass=M, **R.DUST_GEOM)
        c.center = (0.0, 0.0, 0.0)
        c.initData("dust_collapse", **R.DUST_PROB)
        c.gravity.get_new_grav_vector(0)
        torch.cuda.synchronize()
        out.append((c.radial_gravity(), c.grav_new.cpu().numpy().copy(), c))
    for a, b in zip(out[0][0], out[1][0]):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    c = out[1][2]
    before = out[0][1]
    term = PR.pointmass_term(c.gravbox, c.geom, [0.0, 0.0, 0.0], c.Gconst, M)
    assert np.abs(term).max() > 1e-6 * np.abs(before).max()
    _check_add(hydro, out[1][1], before, term, before + term, "monopole + point mass")


def _accrete(hyd, mod, v0, monkeypatch=None, **kw):
    import castro_amd
    P = _params(mod)
    c = castro_amd.Castro(PR.PM_N, params=P, hydro=hyd, do_grav=True, use_point_mass=True, Gconst=PR.PM_G, point_mass=PR.PM_M,
                          point_mass_fix_solution=True, **kw)
    c.set_state(PR.radial_flow_state(P, v0=v0))
    rec = dict(stale=[], pre=[])
    orig = c._do_advance_with_sources
    c._do_advance_with_sources = lambda *a: (lambda r: (rec["stale"].append(r[2]), r)[1])(orig(*a))
    if monkeypatch is not None:                 # the states the update saw, before the restore
        from castro_amd.hydro import HipHydro
        app = HipHydro.pointmass_apply_mf

        def apply(self, boxes, pm, geom, delta, mass, stream=None):
            torch.cuda.synchronize()
            rec["pre"].append((c.S_old_b.cpu().numpy().copy(), c.S_new_b.cpu().numpy().copy(), float(delta[0]), float(mass[0])))
            app(self, boxes, pm, geom, delta, mass, stream)
        monkeypatch.setattr(HipHydro, "pointmass_apply_mf", apply)
    return c, rec


def _cpu_accretion(oracle, v0, **kw):
    key = ("accrete", v0, tuple(sorted(kw.items())))
    if key not in _CACHE:
        c, rec = _accrete(PR.PointMassOracleBackend(), oracle, v0, **kw)
        dts = [c.step(), c.step()]
        _CACHE[key] = (c.S_new().numpy().copy(), dts, c.point_mass)
    return _CACHE[key]


def test_accretion_restores_the_cube_moves_the_mass_and_estimates_dt_afresh(hydro, oracle, monkeypatch):
    from castro_amd import _lib
    c, rec = _accrete(hydro, _lib, -1.5, monkeypatch)
    dt1 = c.step()
    torch.cuda.synchronize()
    assert len(rec["pre"]) == 1
    So, Sn, d, m0 = rec["pre"][0]
    box = [(c.lo, c.hi, So, c.gbox, Sn, c.gbox)]
    terms = PR.delta_terms(box, c.geom, [0.5, 0.5, 0.5])
    want = PR.delta(box, c.geom, [0.5, 0.5, 0.5])
    assert d > 0.0 and abs(d - want) <= 64 * EPS * np.abs(terms).sum(), (d, want)
    assert m0 == PR.PM_M and c.point_mass == PR.PM_M + d
    S = c.S_new_b.cpu().numpy()
    g = 4 + 6
    cube = (slice(None), slice(g, g + 4), slice(g, g + 4), slice(g, g + 4))
    assert np.array_equal(S[cube], So[cube]) and not np.array_equal(Sn[cube], So[cube])
    # the next dt: computeNewDt from a fresh estTimeStep on the final state; the advance's own estimate saw the cube before
    # the restore, where the CFL-limiting zone sat
    fresh = c.computeNewDt(dt1)
    stale = min(rec["stale"][-1], c.params.change_max * dt1)
    assert stale != fresh
    dt2 = c.step()
    assert dt2 == fresh
    torch.cuda.synchronize()
    want_S, dts, want_m = _cpu_accretion(oracle, -1.5)
    _compare(hydro, c.S_new().cpu().numpy(), want_S, [dt1, dt2], dts, "accretion", bits=False)
    assert abs(c.point_mass - want_m) <= 1e-10 * want_m


def test_outflow_changes_nothing(hydro, monkeypatch):
    from castro_amd import _lib
    c, rec = _accrete(hydro, _lib, 1.5, monkeypatch)
    c.step()
    torch.cuda.synchronize()
    So, Sn, d, m0 = rec["pre"][0]
    assert d < 0.0 and c.point_mass == PR.PM_M
    P = _params(_lib)
    free, _ = PR.pointmass_run(hydro, P, PR.radial_flow_state(P, v0=1.5), steps=1)
    torch.cuda.synchronize()
    assert np.array_equal(c.S_new().cpu().numpy(), free.S_new().cpu().numpy()), "the run without point_mass_fix_solution"


def test_accretion_after_a_retry_restores_the_original_old_state(hydro, oracle, monkeypatch):
    from castro_amd import _lib
    c, rec = _accrete(hydro, _lib, -1.5, monkeypatch, initial_dt=0.03)
    start = c.S_new_b.cpu().numpy().copy()
    c.step()
    torch.cuda.synchronize()
    assert c.nretries >= 1 and c.nsubcycles >= 2 and len(rec["pre"]) == 1
    So, Sn, d, m0 = rec["pre"][0]
    g = 4 + 6
    cube = (slice(None), slice(g, g + 4), slice(g, g + 4), slice(g, g + 4))
    assert d > 0.0 and np.array_equal(So[cube], start[cube]), "S_old is the step's original old state"
    assert np.array_equal(c.S_new_b.cpu().numpy()[cube], start[cube])
    assert c.point_mass == PR.PM_M + d


# ---- 4. CastroAmr ----------------------------------------------------------------------------------------------------------------
AMR_M = 2.0e33


def _amr(make_hydro, params, steps=1, **kw):
    return A.dust_amr_run(make_hydro, params, steps=steps, use_point_mass=True, point_mass=AMR_M, **kw)


def _grav_fabs(a):
    return [np.stack([np.asarray(getattr(lev.boxes[0], n).cpu()) for n in ("grav_old", "grav_new")]) for lev in a.lev]


def _fab_dev(a, b):
    return max(np.abs(a[:, n] - b[:, n]).max() for n in range(3)) / np.abs(b).max()


def test_amr_gravity_fabs_follow_the_cpu_hierarchy(hydro, oracle):
    """16^3 octant + a refined 16^3 patch around the centre, monopole gravity and a point mass, one coarse step: grav_old /
    grav_new of both levels -- coarse-fine ghost zones included, where the coarse level's term and the level's own add up --
    against the hierarchy on the CPU restatement backend"""
    import castro_amd
    from castro_amd import _lib
    if "amr" not in _CACHE:
        P = lambda: oracle.default_params(**R.DUST_PARAMS)
        ref, dts = _amr(PR.PointMassOracleBackend, P())
        ulp, _ = _amr(lambda: PR.PointMassOracleBackend(ulps=1), P())
        plain, _ = A.dust_amr_run(PR.PointMassOracleBackend, P(), steps=1)
        w = _grav_fabs(ref)
        _CACHE["amr"] = (w, dts, [_fab_dev(u, r) for u, r in zip(_grav_fabs(ulp), w)], _grav_fabs(plain))
    want, dts, s, plain = _CACHE["amr"]
    a, gdts = _amr(lambda: castro_amd.HipHydro(0, numerics=hydro.numerics), _lib.default_params(**R.DUST_PARAMS))
    torch.cuda.synchronize()
    assert a.point_mass == AMR_M and a.pm.nupdates == 0
    for l, (g, w) in enumerate(zip(_grav_fabs(a), want)):
        tol = max(1e-10, 100.0 * s[l])
        d = _fab_dev(g, w)
        print("AMR gravity FABs level %d (%s): deviation %.3g, s %.3g, tolerance %.3g" % (l, hydro.numerics, d, s[l], tol))
        assert d <= tol
        # the point mass is visible at that tolerance, in the coarse-fine ghost zones as well
        assert _fab_dev(plain[l], w) > 10.0 * tol
        if l == 1:
            ghost = np.abs(plain[l][:, :, 5, 5, -1] - w[:, :, 5, 5, -1]).max() / np.abs(w).max()
            assert ghost > 10.0 * tol
            assert np.abs(g[:, :, :, :, -1] - w[:, :, :, :, -1]).max() <= tol * np.abs(w).max()
    assert np.allclose(gdts, dts, rtol=1e-10, atol=0.0)


def test_amr_update_on_the_finest_level_only(hydro, monkeypatch):
    import castro_amd
    from castro_amd import _lib
    from castro_amd.hydro import HipHydro
    calls, adds = [], []
    od, oa = HipHydro.pointmass_delta_mf, HipHydro.add_pointmass_mf
    monkeypatch.setattr(HipHydro, "pointmass_delta_mf",
                        lambda self, boxes, pm, geom, delta, stream=None: (calls.append((geom.dx[0], boxes[1])), od(self, boxes, pm, geom, delta, stream))[1])
    monkeypatch.setattr(HipHydro, "add_pointmass_mf",
                        lambda self, fabs, pm, geom, mass, stream=None: (adds.append((geom.dx[0], float(mass[0]))), oa(self, fabs, pm, geom, mass, stream))[1])
    mk = lambda: castro_amd.HipHydro(0, numerics=hydro.numerics)
    a, _ = _amr(mk, _lib.default_params(**R.DUST_PARAMS), point_mass_fix_solution=True)
    torch.cuda.synchronize()
    dx1 = a.lev[1].geom.dx[0]
    assert calls == [(dx1, 1), (dx1, 1)], "level 1 only, once per fine subcycle"
    assert a.pm.nupdates == 2
    pm1 = a.point_mass
    assert pm1 >= AMR_M
    n = len(adds)
    assert [x[0] for x in adds].count(a.lev[0].geom.dx[0]) == 2 and [x[0] for x in adds].count(dx1) == 4
    a.step()
    torch.cuda.synchronize()
    first0 = [x for x in adds[n:] if x[0] == a.lev[0].geom.dx[0]][0]
    assert first0[1] == pm1, "level 0's next gravity construction uses the mass the finest level left"
    # max_level = 1 but no fine level: level 0 is the finest existing level and updates
    del calls[:]
    g = castro_amd.MonopoleGravity(drdxfac=A.AMR_DRDXFAC, center=(0.0, 0.0, 0.0))
    b = castro_amd.CastroAmr(A.AMR_N, params=_lib.default_params(**R.DUST_PARAMS), refine=[("density", "value_greater", 1.e300)],
                             max_level=1, make_hydro=mk, do_grav=True, gravity=g, use_point_mass=True, point_mass=AMR_M,
                             point_mass_fix_solution=True, **R.DUST_GEOM)
    b.initData("dust_collapse", **R.DUST_PROB)
    b.step()
    torch.cuda.synchronize()
    assert len(b.lev) == 1 and calls == [(b.lev[0].geom.dx[0], 1)] and b.pm.nupdates == 1

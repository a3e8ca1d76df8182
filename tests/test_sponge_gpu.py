"""GPU tests of the sponge (k_new_sponge_source and the sponge term of k_sources_apply in castro_amd/csrc/aux_kernels.hip,
Castro(sponge=...), CastroAmr(sponge=...)), for both numerics builds.  Reference: tests/sponge_ref.py.

Tolerances.  `exact`: the same bits wherever no cos is evaluated; in a ramp zone the device cos may differ from glibc's, and
the momentum source may then differ by 8 * 2^-52 * (|U_m - rho v_t| * alpha * |uf - lf| / dt + |Sr|) (a 4-ulp cos through
0.5 (uf - lf) (1 - cos) and |dfac/df| <= alpha, doubled); the energy source SrE = sum_n v_n Sr_n by sum_n |v_n| times that,
plus 4 * 2^-52 * sum_n |v_n Sr_n| for the three products and two sums made from different Sr.  `contract`: 1e-10 of the same
scales.  Drivers: bit for bit where no cos is evaluated (`exact`), 1e-10 of a field's maximum otherwise; the dust collapse by
the convention of tests/test_monopole_gpu.py."""
import os

import numpy as np
import pytest
import torch

from tests import monopole_ref as R
from tests import sponge_ref as S
from tests.util import physical_state

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


# ---- 1. the zone function ------------------------------------------------------------------------------------------------------
LO, HI, NG = (5, 8, 3), (44, 31, 18), 3                  # 40 x 24 x 16 valid zones, not at the origin
DT = 3.7e-3
RAMPS = dict(radius=dict(lower_radius=0.45, upper_radius=0.75), density=dict(lower_density=0.5, upper_density=2.0),
             step=dict(lower_density=1.0, upper_density=1.0), pressure=dict(lower_pressure=0.3, upper_pressure=3.0))
CENTER = (0.3137, 1.1713, 2.6291)
ZONE_CASES = [(which, implicit, (0.0, 0.0, 0.0)) for which in ("radius", "step", "pressure", "all") for implicit in (1, 0)] \
    + [("all", 1, (0.4, -0.3, 0.2)), ("density", 0, (-0.1, 0.2, 0.3))]


def _zone_geom():
    from castro_amd import _lib
    return _lib.make_geom((64, 48, 32), (-1.0, 0.5, 2.0), (2.2, 2.42, 4.0), (2, 2, 2), (2, 2, 2))        # dx = 0.05, 0.04, 0.0625


def _zone_state():
    """rho, T and momenta spread over decades, so that every ramp has zones below, on and above it; NaN in the ghost zones"""
    if "zone" not in _CACHE:
        rng = np.random.default_rng(2026)
        n = tuple(HI[d] - LO[d] + 1 for d in (2, 1, 0))
        U = np.full((8,) + tuple(x + 2 * NG for x in n), np.nan)
        v = (slice(None),) + tuple(slice(NG, NG + x) for x in n)
        rho = 10.0 ** rng.uniform(-1.0, 1.0, size=n)
        T = 10.0 ** rng.uniform(-9.0, -7.0, size=n)                  # p / rho = k T / (mu m_u) between 0.08 and 8
        vel = rng.normal(size=(3,) + n)
        W = np.zeros((8,) + n)
        W[S.URHO], W[S.UTEMP], W[S.UFS] = rho, T, rho * rng.uniform(0.9, 1.0, size=n)
        for k in range(3):
            W[S.UMX + k] = rho * vel[k]
        W[S.UEINT] = rho * 1.0
        W[S.UEDEN] = W[S.UEINT] + 0.5 * rho * (vel ** 2).sum(axis=0)
        U[v] = W
        gb = (tuple(x - NG for x in LO), tuple(x + NG for x in HI))
        base = rng.normal(size=(7,) + U.shape[1:])                   # what the source FAB holds before the call
        for k in (S.UMX, S.UMY, S.UMZ, S.UEDEN):
            base[(k,) + v[1:]] = 0.0
        _CACHE["zone"] = dict(U=U, gb=gb, base=base, valid=v)
    return _CACHE["zone"]


def _zone_sponge(which, implicit, vt):
    from castro_amd import _lib
    kw = {}
    for name in (("radius", "density", "pressure") if which == "all" else (which,)):
        kw.update(RAMPS[name])
    return _lib.make_sponge(2.e-3, lower_factor=0.125, upper_factor=0.875, target_velocity=vt, center=CENTER, implicit=implicit, **kw)


def _zone_reference(which, implicit, vt, params):
    key = ("zone", which, implicit, vt)
    if key not in _CACHE:
        c, sp, info = _zone_state(), _zone_sponge(which, implicit, vt), {}
        want = S.apply_sponge(c["U"], c["gb"], LO, HI, sp, _zone_geom(), params, DT, info)
        n = want[0].size
        # at least 10 % of the zones below, on and above every ramp (a step has no "on"), none exactly on a threshold
        rad, u = S.radius(sp, _zone_geom(), LO, HI), c["U"][c["valid"]]
        for name, (below, on, above) in info["region"].items():
            step = which == "step"
            assert below.sum() >= 0.1 * n and above.sum() >= 0.1 * n and (on.sum() == 0 if step else on.sum() >= 0.1 * n), \
                (name, below.sum(), on.sum(), above.sum())
            x = dict(radius=rad, density=u[S.URHO], pressure=info["pressure"])[name]
            lim = dict(radius=(sp.lower_radius, sp.upper_radius), density=(sp.lower_density, sp.upper_density),
                       pressure=(sp.lower_pressure, sp.upper_pressure))[name]
            assert not np.any(x == lim[0]) and not np.any(x == lim[1]), name
        assert set(info["region"]) == (set(("radius", "density", "pressure")) if which == "all" else {which.replace("step", "density")})
        _CACHE[key] = (want, info["cos"].copy(), S.cos_bound(c["U"], c["gb"], LO, HI, sp, want, DT))
    return _CACHE[key]


def _scales(U, want, bound):
    """(4, nz, ny, nx): the bound of the three momentum sources and of the energy source of every zone (module docstring)"""
    v = [np.abs(U[S.UMX + n] * (1.0 / U[S.URHO])) for n in range(3)]
    e = sum(v[n] * bound[n] for n in range(3)) + 4.0 * EPS * sum(v[n] * np.abs(want[S.UMX + n]) for n in range(3))
    return np.concatenate([bound, e[None]])


@pytest.mark.parametrize("which,implicit,vt", ZONE_CASES)
def test_zone_function_against_the_restatement(hydro, oracle, which, implicit, vt):
    from castro_amd import _lib
    P = _lib.default_params()
    c, sp, geom = _zone_state(), _zone_sponge(which, implicit, vt), _zone_geom()
    want, cosm, bound = _zone_reference(which, implicit, vt, oracle.default_params())
    src = _t(c["base"])
    hydro.new_sponge_source(_t(c["U"]), c["gb"], src, c["gb"], LO, HI, sp, geom, P, DT)
    torch.cuda.synchronize()
    got = src.cpu().numpy()
    # ghost zones and the components the sponge does not have keep what they held
    untouched = np.ones(got.shape, dtype=bool)
    for k in (S.UMX, S.UMY, S.UMZ, S.UEDEN):
        untouched[(k,) + c["valid"][1:]] = False
    assert np.array_equal(got[untouched], c["base"][untouched])
    g = got[c["valid"][0:1] + c["valid"][1:]][[S.UMX, S.UMY, S.UMZ, S.UEDEN]]
    w = want[[S.UMX, S.UMY, S.UMZ, S.UEDEN]]
    scale = _scales(c["U"][c["valid"]], want, bound)
    d = np.abs(g - w)
    assert np.abs(w[:3]).max() > 0.0 and (which == "step") == (not cosm.any())
    if hydro.numerics == "exact":
        flat = ~cosm
        assert np.array_equal(g[:, flat], w[:, flat]), "zones without a cos: %d entries differ" % int((g[:, flat] != w[:, flat]).sum())
        ratio = (d[:, cosm] / scale[:, cosm]).max() if cosm.any() else 0.0
        print("sponge zone function (%s, implicit %d, exact): %d ramp zones, largest |device - restatement| / bound = %.3g"
              % (which, implicit, int(cosm.sum()), ratio))
        assert ratio <= 1.0, ratio
    else:
        ratio = (d / (scale / (8.0 * EPS))).max()
        print("sponge zone function (%s, implicit %d, contract): largest deviation / scale = %.3g" % (which, implicit, ratio))
        assert ratio <= 1e-10, ratio


def test_four_unequal_boxes_through_the_one_pass_call(hydro):
    """the same zones cut at x = 13 | 14 and y = 7 | 8 of the box into four FABs of their own, sponge alone, one
    castro_amd_sources_mf_opts call: the source bits of the single-box call"""
    from castro_amd import _lib
    P = _lib.default_params()
    c, sp, geom = _zone_state(), _zone_sponge("all", 1, (0.4, -0.3, 0.2)), _zone_geom()
    one = torch.zeros((7,) + c["U"].shape[1:], dtype=torch.float64, device="cuda")
    hydro.new_sponge_source(_t(c["U"]), c["gb"], one, c["gb"], LO, HI, sp, geom, P, DT)
    one = one.cpu().numpy()
    specs, keep = [], []
    for (x0, x1) in ((LO[0], LO[0] + 12), (LO[0] + 13, HI[0])):
        for (y0, y1) in ((LO[1], LO[1] + 6), (LO[1] + 7, HI[1])):
            lo, hi = (x0, y0, LO[2]), (x1, y1, HI[2])
            gb = (tuple(x - NG for x in lo), tuple(x + NG for x in hi))
            sub = np.ascontiguousarray(c["U"][(slice(None),) + R._sl(c["gb"], lo, hi)])
            F = np.full((8,) + tuple(gb[1][a] - gb[0][a] + 1 for a in (2, 1, 0)), np.nan)
            F[(slice(None),) + R._sl(gb, lo, hi)] = sub
            Sn, So = _t(F), _t(F)
            src = torch.full((7,) + F.shape[1:], 7.0, dtype=torch.float64, device="cuda")
            keep.append((lo, hi, gb, src, Sn, sub))
            specs.append((lo, hi, (So, gb), (Sn, gb), (src, gb), [None] * 3, [(lo, hi)] * 3))
    hydro.sources_mf(1, hydro.make_source_boxes(specs), None, 4, None, geom, P, DT, ntimes=0, sponge=sp)
    torch.cuda.synchronize()
    for lo, hi, gb, src, Sn, sub in keep:
        got = src.cpu().numpy()
        v = (slice(None),) + R._sl(gb, lo, hi)
        assert np.array_equal(got[v], one[(slice(None),) + R._sl(c["gb"], lo, hi)]), (lo, hi)
        ghost = np.ones(got.shape, dtype=bool)
        ghost[v] = False
        assert np.all(got[ghost] == 0.0)
        # the apply: S_new += dt * source on the valid zones (no clean_state), nothing else
        new = Sn.cpu().numpy()[v]
        assert np.array_equal(new[[S.URHO, S.UEINT, S.UTEMP, S.UFS]], sub[[S.URHO, S.UEINT, S.UTEMP, S.UFS]])
        upd = sub[1:5] + DT * got[v][1:5]
        assert np.abs(new[1:5] - upd).max() <= 4.0 * EPS * np.abs(upd).max()


# ---- 2. one pass against separate calls ----------------------------------------------------------------------------------------
def _stage_case():
    if "stage" not in _CACHE:
        rng = np.random.default_rng(5)
        lo, hi = (0, 0, 0), (23, 19, 15)
        gb = (tuple(x - 4 for x in lo), tuple(x + 4 for x in hi))
        sb = (tuple(x - 3 for x in lo), tuple(x + 3 for x in hi))
        vb = (tuple(x - 1 for x in lo), tuple(x + 1 for x in hi))
        UO, UN = physical_state(rng, gb[0], gb[1], jump=True), physical_state(rng, gb[0], gb[1], jump=True)
        fb, M = [], []
        for d in range(3):
            fhi = list(hi)
            fhi[d] += 1
            fb.append((lo, tuple(fhi)))
            M.append(rng.normal(size=(1,) + tuple(fhi[a] - lo[a] + 1 for a in (2, 1, 0))))
        g = [rng.uniform(-1.0, 1.0, size=(3,) + tuple(vb[1][a] - vb[0][a] + 1 for a in (2, 1, 0))) for _ in range(2)]
        _CACHE["stage"] = dict(lo=lo, hi=hi, gb=gb, sb=sb, vb=vb, UO=UO, UN=UN, fb=fb, M=M, gold=g[0], gnew=g[1],
                               sshape=(7,) + tuple(sb[1][a] - sb[0][a] + 1 for a in (2, 1, 0)))
    return _CACHE["stage"]


@pytest.mark.parametrize("form", ["vector+rotation", "gravity FABs"])
def test_one_pass_equals_separate_calls(hydro, form):
    """stage 1 with the sponge last: the Source_Type FAB and S_new of the one-pass kernel carry the bits of the separate calls,
    in both builds"""
    from castro_amd import _lib
    c, dt, gtype = _stage_case(), 0.013, 4
    geom = _lib.make_geom((24, 20, 16), prob_hi=(3.0, 2.5, 2.0))
    P = _lib.default_params()
    sp = _lib.make_sponge(5.e-3, lower_radius=0.8, upper_radius=1.6, lower_density=0.5, upper_density=1.2, center=(1.4, 1.3, 0.9))
    rot = _lib.make_rotation(1.5, center=(1.5, 1.25, 1.0)) if form == "vector+rotation" else None
    vec = (0.3, -0.7, -9.8)
    lo, hi, gb, sb = c["lo"], c["hi"], c["gb"], c["sb"]
    UO, M, go, gn = _t(c["UO"]), [_t(m) for m in c["M"]], _t(c["gold"]), _t(c["gnew"])
    # separate calls
    Un, src = _t(c["UN"]), torch.zeros(c["sshape"], dtype=torch.float64, device="cuda")
    if rot is not None:
        hydro.new_gravity_source(UO, gb, Un, gb, src, sb, M, c["fb"], lo, hi, vec, gtype, dt, geom)
        hydro.new_rotation_source(UO, gb, Un, gb, src, sb, M, c["fb"], lo, hi, rot, geom, dt)
    else:
        hydro.new_gravity_source_gfab(UO, gb, Un, gb, src, sb, M, c["fb"], lo, hi, go, gn, c["vb"], gtype, dt, geom)
    before = src.clone()
    hydro.new_sponge_source(Un, gb, src, sb, lo, hi, sp, geom, P, dt)
    hydro.apply_source(Un, gb, Un, gb, dt, src, sb, 7, lo, hi, P, ntimes=1)
    # one pass
    Un1, src1 = _t(c["UN"]), torch.full(c["sshape"], 3.0, dtype=torch.float64, device="cuda")
    boxes = hydro.make_source_boxes([(lo, hi, (UO, gb), (Un1, gb), (src1, sb), M, c["fb"])])
    if rot is not None:
        hydro.sources_mf(1, boxes, vec, gtype, rot, geom, P, dt, ntimes=1, sponge=sp)
    else:
        hydro.sources_mf_g(1, boxes, hydro.make_grav_fabs([(go, c["vb"])]), hydro.make_grav_fabs([(gn, c["vb"])]), gtype, None, geom,
                           P, dt, ntimes=1, sponge=sp)
    torch.cuda.synchronize()
    assert not torch.equal(before, src), "the sponge adds something"
    v = (slice(None),) + R._sl(gb, lo, hi)
    assert torch.equal(src1, src), "source: %d entries differ" % int((src1 != src).sum())
    assert torch.equal(Un1[v], Un[v]), "S_new: %d entries differ" % int((Un1[v] != Un[v]).sum())
    # stage 0 takes a sponge and adds nothing: the call without one
    outs = []
    for kw in ({}, {"sponge": sp}):
        Un0, src0 = _t(c["UN"]), torch.full(c["sshape"], 3.0, dtype=torch.float64, device="cuda")
        b0 = hydro.make_source_boxes([(lo, hi, (UO, gb), (Un0, gb), (src0, sb), M, c["fb"])])
        if rot is not None:
            hydro.sources_mf(0, b0, vec, gtype, rot, geom, P, dt, ntimes=1, **kw)
        else:
            hydro.sources_mf_g(0, b0, hydro.make_grav_fabs([(go, c["vb"])]), hydro.make_grav_fabs([(gn, c["vb"])]), gtype, None,
                               geom, P, dt, ntimes=1, **kw)
        outs.append((src0, Un0[v].clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_argument_checks(hydro):
    from castro_amd import _lib
    c, P = _zone_state(), _lib.default_params()
    sp, geom = _zone_sponge("radius", 1, (0.0, 0.0, 0.0)), _zone_geom()
    U, src = _t(c["U"]), torch.zeros((7,) + c["U"].shape[1:], dtype=torch.float64, device="cuda")
    bad_t = _lib.Sponge.from_buffer_copy(sp)
    bad_t.timescale = 0.0
    bad_g = _lib.Geom.from_buffer_copy(geom)
    bad_g.coord = 1
    for s, g, dt in ((bad_t, geom, DT), (sp, bad_g, DT), (sp, geom, 0.0)):
        with pytest.raises(RuntimeError):
            hydro.new_sponge_source(U, c["gb"], src, c["gb"], LO, HI, s, g, P, dt)
        boxes = hydro.make_source_boxes([(LO, HI, (U, c["gb"]), (U, c["gb"]), (src, c["gb"]), [None] * 3, [(LO, HI)] * 3)])
        with pytest.raises(RuntimeError):
            hydro.sources_mf(1, boxes, None, 4, None, g, P, dt, ntimes=0, sponge=s)
    torch.cuda.synchronize()
    assert np.all(src.cpu().numpy() == 0.0)


# ---- 3. / 4. Sedov -------------------------------------------------------------------------------------------------------------
SEDOV = dict(step=dict(lower_density=0.99, upper_density=0.99), radial=dict(lower_radius=0.05, upper_radius=0.3))


def _sedov(hyd, params, sponge, steps=3):
    import castro_amd
    c = castro_amd.Castro((16, 16, 16), params=params, hydro=hyd, sponge=sponge)
    c.initData("sedov", r_init=0.1, nsub=4)
    return c, [c.step() for _ in range(steps)]


def _sedov_reference(oracle, kind):
    from castro_amd import _lib
    if ("sedov", kind) not in _CACHE:
        P = lambda: oracle.default_params(init_shrink=0.1)
        sp = None if kind == "none" else _lib.make_sponge(1.e-3, **SEDOV[kind])
        c, dts = _sedov(S.SpongeOracleBackend(), P(), sp)
        if kind == "step":
            one, _ = _sedov(S.SpongeOracleBackend(), P(), _lib.make_sponge(1.e-3, **SEDOV[kind]), steps=1)
            u = one.S_new().numpy()
            moving = np.abs(u[S.UMX:S.UMZ + 1]).max(axis=0) > 0.0
            assert (moving & (u[S.URHO] < 0.99)).sum() > 0 and (moving & (u[S.URHO] > 0.99)).sum() > 0
            assert not np.any(u[S.URHO] == 0.99)
        _CACHE[("sedov", kind)] = (c.S_new().numpy().copy(), dts)
    return _CACHE[("sedov", kind)]


def test_sedov_with_a_density_step_sponge(hydro, oracle):
    """16^3, three steps, sponge_lower_density = sponge_upper_density = 0.99 (after one step the blast has moving zones
    between 0.97 and 1.01): no cos anywhere, so `exact` is the CPU driver bit
    for bit; `contract` within 1e-10 per field; and the sponge changes the run"""
    from castro_amd import _lib
    want, dts = _sedov_reference(oracle, "step")
    free, _ = _sedov_reference(oracle, "none")
    c, gdts = _sedov(hydro, _lib.default_params(init_shrink=0.1), _lib.make_sponge(1.e-3, **SEDOV["step"]))
    torch.cuda.synchronize()
    got = c.S_new().cpu().numpy()
    d = R.field_deviation(got, want)
    print("Sedov with a density step sponge (%s): deviation per field" % hydro.numerics, d)
    if hydro.numerics == "exact":
        assert np.array_equal(got, want), "%d entries differ, deviation per field %s" % (int((got != want).sum()), d)
        assert gdts == dts
    else:
        assert np.all(d <= 1e-10), d
        assert np.allclose(gdts, dts, rtol=1e-10, atol=0.0)
    assert R.field_deviation(got, free)[S.UMX] > 1e-3


def test_sedov_with_a_radial_ramp_through_the_blast(hydro, oracle):
    from castro_amd import _lib
    want, dts = _sedov_reference(oracle, "radial")
    c, gdts = _sedov(hydro, _lib.default_params(init_shrink=0.1), _lib.make_sponge(1.e-3, **SEDOV["radial"]))
    torch.cuda.synchronize()
    d = R.field_deviation(c.S_new().cpu().numpy(), want)
    print("Sedov with a radial sponge ramp (%s): deviation per field" % hydro.numerics, d)
    assert np.all(d <= 1e-10), d
    assert np.allclose(gdts, dts, rtol=1e-10, atol=0.0)


# ---- 5. dust collapse ----------------------------------------------------------------------------------------------------------
def dust_sponge():
    """castro.do_sponge = 1 of Exec/gravity_tests/DustCollapse/inputs_3d_monopole_regtest"""
    from castro_amd import _lib
    return _lib.make_sponge(1.e-3, lower_density=1.e-3, upper_density=1.e-3)


def _ambient_deviation(a, b, amb):
    """the deviation of the momenta of the ambient zones over the largest momentum among them, and of the other fields likewise"""
    return R.field_deviation(np.where(amb[None], a, 0.0), np.where(amb[None], b, 0.0))


def test_dust_collapse_with_the_regression_sponge(hydro, oracle):
    """The dust collapse of tests/test_monopole_gpu.py with the sponge of the regression input.  Tolerance per field:
    max(1e-10, 100 s), s the deviation of a CPU run whose radial masses differ by one ulp per bin, with the sponge on; the
    same again on the ambient zones alone (rho < 1e-3), each field over its largest magnitude among those zones -- the ambient
    momentum is some 1e-14 of the star's and invisible in the whole-field norm."""
    from castro_amd import _lib
    if "dust" not in _CACHE:
        P = lambda: oracle.default_params(**R.DUST_PARAMS)
        ref, dts = R.dust_collapse_run(S.SpongeOracleBackend(), P(), sponge=dust_sponge())
        ulp, _ = R.dust_collapse_run(S.SpongeOracleBackend(ulps=1), P(), sponge=dust_sponge())
        free, _ = R.dust_collapse_run(S.SpongeOracleBackend(), P())
        w, u = ref.S_new().numpy().copy(), ulp.S_new().numpy()
        amb = w[S.URHO] < 1.e-3
        assert amb.sum() > 100 and not np.any(w[S.URHO] == 1.e-3)
        _CACHE["dust"] = (w, dts, R.field_deviation(u, w), amb, _ambient_deviation(u, w, amb), free.S_new().numpy().copy())
    want, dts, s, amb, s_amb, free = _CACHE["dust"]
    c, gdts = R.dust_collapse_run(hydro, _lib.default_params(**R.DUST_PARAMS), sponge=dust_sponge())
    torch.cuda.synchronize()
    got = c.S_new().cpu().numpy()
    tol, tol_amb = np.maximum(1e-10, 100.0 * s), np.maximum(1e-10, 100.0 * s_amb)
    d, d_amb = R.field_deviation(got, want), _ambient_deviation(got, want, amb)
    print("dust collapse with sponge (%s): s" % hydro.numerics, s, "deviation", d, "tolerance", tol)
    print("dust collapse with sponge (%s), %d ambient zones: s" % (hydro.numerics, amb.sum()), s_amb, "deviation", d_amb,
          "tolerance", tol_amb)
    assert np.all(d <= tol), (d, tol)
    assert np.all(d_amb <= tol_amb), (d_amb, tol_amb)
    assert np.allclose(np.array(gdts), np.array(dts), rtol=1e-12, atol=0.0), (gdts, dts)
    assert _ambient_deviation(got, free, amb)[S.UMX] > 1e4 * tol_amb[S.UMX], "the sponge acts on the ambient gas"


# ---- 6. CastroAmr --------------------------------------------------------------------------------------------------------------
def _amr_run(make_hydro, params, steps=2):
    import castro_amd
    from castro_amd import _lib
    a = castro_amd.CastroAmr((16, 16, 16), patch_crse=((4, 4, 4), (11, 11, 11)), params=params, make_hydro=make_hydro,
                             sponge=_lib.make_sponge(1.e-3, **SEDOV["radial"]))
    a.initData("sedov", r_init=0.1, nsub=4)
    return a, [a.step() for _ in range(steps)]


def _levels(a):
    return [lev.boxes[0].S_new().cpu().numpy() for lev in a.levels]


def test_amr_level_calls_per_box_calls_and_the_cpu_driver(hydro, oracle, monkeypatch):
    """base 16^3 + a fixed 2x patch, radial sponge, two coarse steps: the sponge inside the level's one-pass call and as a
    call per box give the same bits; both builds follow the CPU hierarchy within 1e-10 of every field's maximum"""
    import castro_amd
    from castro_amd import _lib
    from castro_amd.hydro import HipHydro
    if "amr" not in _CACHE:
        ref, dts = _amr_run(S.SpongeOracleBackend, oracle.default_params(init_shrink=0.1))
        _CACHE["amr"] = (_levels(ref), dts)
    want, dts = _CACHE["amr"]
    calls = []
    orig = HipHydro.new_sponge_source
    monkeypatch.setattr(HipHydro, "new_sponge_source", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    mk = lambda: castro_amd.HipHydro(0, numerics=hydro.numerics)
    a, gdts = _amr_run(mk, _lib.default_params(init_shrink=0.1))
    torch.cuda.synchronize()
    one = _levels(a)
    # a base level that is one plain Castro box advances box by box (it has no level tables): its two advances are separate
    # calls; the four advances of the fine level carry the sponge inside the level's one-pass call
    n_one = len(calls)
    assert n_one == 2, n_one
    monkeypatch.setenv("CASTRO_AMD_SOURCES_ONE_PASS", "0")
    b, bdts = _amr_run(mk, _lib.default_params(init_shrink=0.1))
    torch.cuda.synchronize()
    print("AMR sponge (%s): separate new_sponge_source calls: %d in the default run, %d with CASTRO_AMD_SOURCES_ONE_PASS=0"
          % (hydro.numerics, n_one, len(calls) - n_one))
    # two coarse steps are two advances of level 0 and four of level 1: box by box that is one call each
    assert len(calls) - n_one == 2 * (1 + 2), (n_one, len(calls))
    for l, (x, y) in enumerate(zip(one, _levels(b))):
        assert np.array_equal(x, y), "level %d: %d entries differ between the level call and the per-box calls" % (l, int((x != y).sum()))
    assert gdts == bdts
    for l, (x, w) in enumerate(zip(one, want)):
        d = R.field_deviation(x, w)
        print("AMR Sedov with a radial sponge (%s) level %d: deviation per field" % (hydro.numerics, l), d)
        assert np.all(d <= 1e-10), (l, d)
    assert np.allclose(gdts, dts, rtol=1e-10, atol=0.0)

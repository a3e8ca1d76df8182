"""GPU tests of explicit thermal diffusion: the HIP kernels against the numpy restatement (tests/diffusion_ref.py) -- the `exact`
build bit for bit, the `contract` build within 1e-10 of the scale of the face contributions -- and the device driver against
the CPU driver (the oracle's clean_state / hydro + the numpy term) on the reference's diffusion_test and on Sedov with
diffusion and gravity."""
import ctypes as C

import numpy as np
import pytest

from tests import diffusion_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-10
MODES = ("exact", "contract")


def _term_case():
    """40 x 24 x 16 valid zones = the domain, 2 ghost zones; periodic x, outflow y, slip wall low z / outflow high z; densities
    across the ramp (cutoff 1, cutoff_hi 2.5) and below the cutoff; the ghost zones behind physical faces hold NaNs"""
    from castro_amd import _lib
    rng = np.random.default_rng(20250)
    n, g = (40, 24, 16), 2
    lo, hi = (0, 0, 0), tuple(x - 1 for x in n)
    box = (tuple(-g for _ in n), tuple(x - 1 + g for x in n))
    U = np.full((8, n[2] + 2 * g, n[1] + 2 * g, n[0] + 2 * g), np.nan)
    v = (slice(None), slice(g, -g), slice(g, -g), slice(g, -g))
    U[v] = rng.uniform(0.5, 3.5, size=(8,) + n[::-1])
    U[R.UTEMP][v[1:]] = rng.uniform(1.0, 2.0, size=n[::-1])
    U[:, g:-g, g:-g, :g] = U[:, g:-g, g:-g, n[0]:n[0] + g]             # the periodic wrap in x
    U[:, g:-g, g:-g, -g:] = U[:, g:-g, g:-g, g:2 * g]
    rho = U[R.URHO][v[1:]]
    assert (rho <= 1.0).mean() > 0.1 and ((rho > 1.0) & (rho < 2.5)).mean() > 0.3 and (rho >= 2.5).mean() > 0.2
    sbox = (tuple(-3 for _ in n), tuple(x + 2 for x in n))
    src = rng.uniform(-1.0, 1.0, size=(7, n[2] + 6, n[1] + 6, n[0] + 6))
    geom = _lib.make_geom(n, lo_bc=(0, 2, 4), hi_bc=(0, 2, 2))
    diff = _lib.make_diffusion(3.0, 1.0, 2.5, 0.7)
    return n, lo, hi, box, U, sbox, src, geom, diff


@pytest.mark.parametrize("mode", MODES)
def test_term_against_the_numpy_restatement(mode):
    import torch
    import castro_amd
    n, lo, hi, box, U, sbox, src, geom, diff = _term_case()
    mult = -0.5
    D, A = R.diffusion_term(U, box, lo, hi, geom, diff)
    assert np.isfinite(D).all() and (A > 0.0).mean() > 0.9
    want = src.copy()
    sv = (slice(3, -3),) * 3
    for m in (R.UEDEN, R.UEINT):
        want[m][sv] = want[m][sv] + mult * D
    h = castro_amd.HipHydro(0, numerics=mode)
    Ud = torch.as_tensor(U, device="cuda")

    def compare(got, gotD, tag):
        for m in range(7):
            if m not in (R.UEDEN, R.UEINT):
                assert np.array_equal(got[m], src[m]), (tag, m)
        assert np.array_equal(got[:, :3], src[:, :3]) and np.array_equal(got[:, :, :, -3:], src[:, :, :, -3:])     # ghost zones untouched
        for m in (R.UEDEN, R.UEINT):
            d = np.abs(got[m][sv] - want[m][sv])
            print("%s %s comp %d: %d of %d zones differ, max |delta| / A = %.3e" % (mode, tag, m, int((d > 0).sum()), d.size,
                                                                                      float((d / np.maximum(A, 1e-300)).max())))
            if mode == "exact":
                assert np.array_equal(got[m][sv], want[m][sv]), (tag, m)
            else:
                assert (d <= RTOL * A).all(), (tag, m)
        if gotD is not None:
            if mode == "exact":
                assert np.array_equal(gotD, D), tag
            else:
                assert (np.abs(gotD - D) <= RTOL * A).all(), tag

    # one box, with the bare term as well
    s = torch.as_tensor(src, device="cuda").clone()
    dt_ = torch.full((1,) + n[::-1], -7.0, dtype=torch.float64, device="cuda")
    h.temp_diffusion(Ud, box, s, sbox, lo, hi, diff, geom, mult, diff_term=dt_, diff_term_box=(lo, hi))
    torch.cuda.synchronize()
    compare(s.cpu().numpy(), dt_.cpu().numpy()[0], "_fab")
    # the bare term alone
    dt2 = torch.zeros_like(dt_)
    h.temp_diffusion(Ud, box, None, None, lo, hi, diff, geom, 1.0, diff_term=dt2, diff_term_box=(lo, hi))
    assert torch.equal(dt2, dt_)
    # four unequal boxes of the same FABs in one launch
    s = torch.as_tensor(src, device="cuda").clone()
    cuts = [((0, 0, 0), (12, 9, 15)), ((13, 0, 0), (39, 9, 15)), ((0, 10, 0), (12, 23, 15)), ((13, 10, 0), (39, 23, 15))]
    h.temp_diffusion_mf(h.make_diffusion_boxes([(a, b, (Ud, box), (s, sbox)) for a, b in cuts]), diff, geom, mult)
    torch.cuda.synchronize()
    compare(s.cpu().numpy(), None, "_mf")
    h.close()


def test_unsupported_boundaries_and_geometry_are_refused():
    import torch
    import castro_amd
    from castro_amd import _lib
    n, lo, hi, box, U, sbox, src, geom, diff = _term_case()
    h = castro_amd.HipHydro(0)
    Ud, s = torch.as_tensor(U, device="cuda"), torch.as_tensor(src, device="cuda")
    none = _lib.fab_desc(None, lo, hi, 0)
    cases = [dict(lo_bc=(1, 2, 2)), dict(hi_bc=(2, 3, 2)), dict(lo_bc=(2, 2, 1), hi_bc=(2, 2, 3))]
    geoms = [_lib.make_geom(n, **kw) for kw in cases]
    cyl = _lib.make_geom(n)
    cyl.coord = 1
    for g in geoms + [cyl]:
        rc = h.lib.castro_amd_temp_diffusion_fab(h.h, C.byref(_lib.fab_of(Ud, *box)), C.byref(_lib.fab_of(s, *sbox)), C.byref(none),
                                                 _lib.i3(lo), _lib.i3(hi), C.byref(diff), C.byref(g), 1.0, None)
        assert rc == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy(), src)
    # a state without a ghost zone around [lo, hi] is an argument error
    rc = h.lib.castro_amd_temp_diffusion_fab(h.h, C.byref(_lib.fab_of(Ud, *box)), C.byref(_lib.fab_of(s, *sbox)), C.byref(none),
                                             _lib.i3((-2, 0, 0)), _lib.i3(hi), C.byref(diff), C.byref(geom), 1.0, None)
    assert rc == _lib.ERR_ARG
    h.close()


@pytest.mark.parametrize("mode", MODES)
def test_estdt_temp_diffusion_against_numpy(mode):
    import torch
    import castro_amd
    from castro_amd import _lib
    from tests.util import physical_state
    rng = np.random.default_rng(7)
    lo, hi = (0, 0, 0), (47, 29, 21)
    U = physical_state(rng, lo, hi, smooth=False)
    geom = _lib.make_geom((48, 30, 22), prob_hi=(1.0, 0.5, 0.7))
    P = _lib.default_params(cfl=0.3)
    diff = _lib.make_diffusion(2.5e7, 0.5)                  # the jump of physical_state puts a good share of the zones below 0.5
    assert 0.1 < (U[0] <= 0.5).mean() < 0.9
    want = R.estdt_temp_diffusion(U, (lo, hi), lo, hi, geom, P, diff, 1.e200)
    h = castro_amd.HipHydro(0, numerics=mode)
    Ud = torch.as_tensor(U, device="cuda")
    for form in ("fab", "mf"):
        out = torch.full((1,), 1.e300, dtype=torch.float64, device="cuda")
        if form == "fab":
            h.estdt_temp_diffusion(Ud, (lo, hi), lo, hi, geom, P, diff, 1.e200, out)
        else:
            h.estdt_temp_diffusion_mf(h.make_state_boxes([((0, 0, 0), (47, 29, 9), (Ud, (lo, hi))), ((0, 0, 10), (47, 29, 21), (Ud, (lo, hi)))]),
                                      geom, P, diff, 1.e200, out)
        got = out.item()
        print("%s estdt_temp_diffusion_%s: %.17g (numpy %.17g)" % (mode, form, got, want))
        if mode == "exact":
            assert got == want
        else:
            assert abs(got - want) <= RTOL * want
    # a box entirely below the cutoff: max_dt / cfl
    out = torch.full((1,), 1.e300, dtype=torch.float64, device="cuda")
    h.estdt_temp_diffusion(Ud, (lo, hi), lo, hi, geom, P, _lib.make_diffusion(2.5e7, 1.e3), 5.0, out)
    assert out.item() == 5.0 / 0.3
    h.close()


def _state_deviation(got, want):
    """the checker of the `contract` driver runs, on the conserved state: max |delta| of a component over its scale (the
    component's own maximum; the three momenta share the largest of theirs; a field that is zero is compared absolutely)"""
    mom = max(np.abs(want[k]).max() for k in (1, 2, 3))
    dev = {}
    for k in range(8):
        scale = mom if k in (1, 2, 3) else np.abs(want[k]).max()
        d = np.abs(got[k] - want[k]).max()
        dev[k] = d / scale if scale > 0.0 else d
    return dev


def _compare_step(mode, tag, c, ref):
    import torch
    torch.cuda.synchronize()
    got, want = c.S_new().cpu().numpy(), ref.S_new().numpy()
    if mode == "exact":
        assert c.dt == ref.dt, (tag, c.nstep, c.dt, ref.dt)
        for k in range(8):
            assert np.array_equal(got[k], want[k]), "%s: component %d differs after step %d" % (tag, k, c.nstep)
        return 0.0
    dev = _state_deviation(got, want)
    bad = {k: v for k, v in dev.items() if not v <= RTOL}
    assert not bad, "%s step %d: components beyond rtol %g: %s" % (tag, c.nstep, RTOL, bad)
    assert abs(c.dt - ref.dt) <= RTOL * ref.dt and abs(c.time - ref.time) <= RTOL * max(ref.time, ref.dt)
    return max(dev.values())


DT_PARAMS = dict(cfl=0.3, init_shrink=0.1, change_max=1.1)


@pytest.mark.parametrize("mode", MODES)
def test_diffusion_test_32_on_the_device_follows_the_cpu_driver(oracle, mode):
    import castro_amd
    n, stop = (32, 32, 32), 1.e-3
    c = castro_amd.Castro(n, params=castro_amd.default_params(**DT_PARAMS), numerics=mode, do_hydro=False,
                          diffusion=castro_amd.make_diffusion(10.0))
    ref = castro_amd.Castro(n, params=oracle.default_params(**DT_PARAMS), hydro=R.DiffusionOracleBackend(), do_hydro=False,
                            diffusion=castro_amd.make_diffusion(10.0))
    worst = 0.0
    for x in (c, ref):
        x.initData("diffusion_test")
    _compare_step(mode, "diffusion_test", c, ref)
    while ref.time < stop - 1e-18:
        c.step(stop)
        ref.step(stop)
        assert c.dt_limiter == ref.dt_limiter == "diffusion"
        worst = max(worst, _compare_step(mode, "diffusion_test", c, ref))
    assert c.nstep == ref.nstep == 22
    print("%s diffusion_test 32^3: %d steps, worst deviation from the CPU driver %.2e" % (mode, c.nstep, worst))
    c.close()


def test_diffusion_test_64_contract_against_the_analytic_gaussian():
    import torch
    import castro_amd
    c = castro_amd.Castro((64, 64, 64), params=castro_amd.default_params(**DT_PARAMS), numerics="contract", do_hydro=False,
                          diffusion=castro_amd.make_diffusion(10.0))
    c.initData("diffusion_test")
    c.evolve(1.e-3)
    torch.cuda.synchronize()
    err = float(np.abs(c.S_new()[R.UTEMP].cpu().numpy() - c.diffusion_test_analytic(c.time)).max())
    print("contract diffusion_test 64^3: %d steps, Linf(Temp) = %.6e" % (c.nstep, err))
    assert abs(c.time - 1.e-3) <= 1e-15
    assert abs(err - 3.99e-3) <= 0.02 * 3.99e-3
    c.close()


@pytest.mark.parametrize("one_pass", ("1", "0"))
@pytest.mark.parametrize("mode", MODES)
def test_sedov_with_diffusion_and_gravity_follows_the_cpu_driver(oracle, monkeypatch, mode, one_pass):
    """hydro + diffusion + constant gravity: the order diffusion -> gravity in UEDEN, through the one-pass source path
    (castro_amd_sources_mf_ex) and through the separate calls"""
    import castro_amd
    monkeypatch.setenv("CASTRO_AMD_SOURCES_ONE_PASS", one_pass)
    n = (32, 32, 32)
    kw = dict(do_grav=True, const_grav=-0.5, diffusion=castro_amd.make_diffusion(1.e9))
    c = castro_amd.Castro(n, numerics=mode, **kw)
    ref = castro_amd.Castro(n, params=oracle.default_params(), hydro=R.DiffusionOracleBackend(), **kw)
    for x in (c, ref):
        x.initData("sedov", r_init=0.12, nsub=3)
    worst = 0.0
    for _ in range(10):
        c.step()
        ref.step()
        worst = max(worst, _compare_step(mode, "sedov+diffusion+gravity", c, ref))
    print("%s one_pass=%s sedov + diffusion + gravity 32^3: 10 steps, worst deviation %.2e, limiter %s" % (mode, one_pass, worst, c.dt_limiter))
    c.close()

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
    # the other argument checks: each is CASTRO_AMD_ERR_ARG and writes nothing
    term = np.full((1,) + n[::-1], -7.0)
    t = torch.as_tensor(term, device="cuda")
    s5, t2, U7 = s[:5].contiguous(), torch.full((2,) + n[::-1], -7.0, dtype=torch.float64, device="cuda"), Ud[:7].contiguous()
    inner = ((1, 0, 0), hi)                                 # a FAB that misses the plane i = 0 of [lo, hi]
    t_in = torch.full((1, n[2], n[1], n[0] - 1), -7.0, dtype=torch.float64, device="cuda")
    s_in = torch.full((7, n[2], n[1], n[0] - 1), -7.0, dtype=torch.float64, device="cuda")
    fab = _lib.fab_of
    refused = {"source with 5 components": (fab(Ud, *box), fab(s5, *sbox), none),
               "diff_term with 2 components": (fab(Ud, *box), fab(s, *sbox), fab(t2, lo, hi)),
               "diff_term box not containing [lo, hi]": (fab(Ud, *box), fab(s, *sbox), fab(t_in, *inner)),
               "source box not containing [lo, hi]": (fab(Ud, *box), fab(s_in, *inner), fab(t, lo, hi)),
               "source and diff_term both NULL": (fab(Ud, *box), none, none),
               "state with 7 components": (fab(U7, *box), fab(s, *sbox), fab(t, lo, hi))}
    for what, (fu, fs, ft) in refused.items():
        rc = h.lib.castro_amd_temp_diffusion_fab(h.h, C.byref(fu), C.byref(fs), C.byref(ft), _lib.i3(lo), _lib.i3(hi), C.byref(diff),
                                                 C.byref(geom), 1.0, None)
        assert rc == _lib.ERR_ARG, what
    rc = h.lib.castro_amd_temp_diffusion_fab(h.h, C.byref(fab(Ud, *box)), None, None, _lib.i3(lo), _lib.i3(hi), C.byref(diff), C.byref(geom), 1.0, None)
    assert rc == _lib.ERR_ARG
    # _mf: the second box of the table has no source
    arr, nb = h.make_diffusion_boxes([((0, 0, 0), (12, 23, 15), (Ud, box), (s, sbox)), ((13, 0, 0), (39, 23, 15), (Ud, box), (s, sbox))])
    arr[1].source = _lib.fab_desc(None, sbox[0], sbox[1], 7)
    assert h.lib.castro_amd_temp_diffusion_mf(h.h, nb, arr, C.byref(diff), C.byref(geom), 1.0, None) == _lib.ERR_ARG
    # an empty box (hi < lo in one direction) is no error: nothing is launched
    rc = h.lib.castro_amd_temp_diffusion_fab(h.h, C.byref(fab(Ud, *box)), C.byref(fab(s, *sbox)), C.byref(fab(t, lo, hi)), _lib.i3(lo),
                                             _lib.i3((hi[0], -1, hi[2])), C.byref(diff), C.byref(geom), 1.0, None)
    assert rc == _lib.OK
    torch.cuda.synchronize()
    assert h.status() == 0
    assert np.array_equal(s.cpu().numpy(), src) and np.array_equal(t.cpu().numpy(), term) and np.array_equal(Ud.cpu().numpy(), U, equal_nan=True)
    assert np.array_equal(s5.cpu().numpy(), src[:5]) and (t2 == -7.0).all() and (t_in == -7.0).all() and (s_in == -7.0).all()
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


# ---- unit tests of the kernels at the shapes where they can go wrong ----------------------------------------------------------
# k_temp_diffusion tiles a box as 64 (i) x 4 (j) x 32 (k); a thread restarts its column at every k-chunk, and the workgroups are
# renumbered over the 8 XCDs.  The index space below starts away from zero and is anisotropic, and the three FABs of a call have
# different ghost widths, hence different strides.
TILE = (64, 4, 32)
DOMLO = (-5, 3, 100)
DX = (0.02, 0.1, 0.0125)
PROB_LO = (0.0, -1.0, 2.0)
BC_LO, BC_HI = (0, 2, 4), (0, 2, 2)                        # periodic x, outflow y, slip wall low z / outflow high z


def _geom(dom_n, domlo, lo_bc=BC_LO, hi_bc=BC_HI):
    from castro_amd import _lib
    return _lib.make_geom(dom_n, prob_lo=PROB_LO, prob_hi=tuple(PROB_LO[d] + DX[d] * dom_n[d] for d in range(3)), lo_bc=lo_bc, hi_bc=hi_bc,
                          domlo=domlo)


def _diff():
    from castro_amd import _lib
    return _lib.make_diffusion(3.0, 1.0, 2.5, 0.7)


def _blocks(n):
    return int(np.prod([(n[d] + TILE[d] - 1) // TILE[d] for d in range(3)]))


def _placed(n, placement):
    """[lo, hi] of n valid zones from DOMLO and the geometry that puts it: the whole domain / strictly inside a larger one (no face
    is physical) / in the low-x, high-z corner of a larger one with outflow all round (two faces physical, four interior)"""
    lo, hi = DOMLO, tuple(DOMLO[d] + n[d] - 1 for d in range(3))
    if placement == "domain":
        return lo, hi, _geom(n, lo)
    if placement == "inside":
        return lo, hi, _geom(tuple(x + 16 for x in n), tuple(x - 8 for x in lo))
    assert placement == "low-x-high-z"
    return lo, hi, _geom((n[0] + 8, n[1] + 16, n[2] + 8), (lo[0], lo[1] - 8, lo[2] - 8), lo_bc=(2, 2, 2), hi_bc=(2, 2, 2))


def _assert_density_shares(rho):
    """at or below the cutoff, on the ramp, at or above cutoff_hi: the shares of the unit case where the box has the zones for
    them, every class present in a small one, nothing to ask of a single zone"""
    below, ramp, above = rho <= 1.0, (rho > 1.0) & (rho < 2.5), rho >= 2.5
    if rho.size >= 512:
        assert below.mean() > 0.1 and ramp.mean() > 0.3 and above.mean() > 0.2
    elif rho.size > 1:
        assert below.any() and ramp.any() and above.any()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").clone()


def _compare(mode, got, want, scale, tag):
    """the module's rule: `exact` bit for bit, `contract` |delta| <= RTOL * scale zone by zone (a NaN fails both)"""
    assert np.isfinite(want).all(), tag
    d = np.abs(got - want)
    with np.errstate(all="ignore"):
        worst = float(np.where(d > 0, d / np.maximum(scale, 1e-300), 0.0).max()) if d.size else 0.0
    msg = "%s %s: %d of %d zones differ, max |delta| / scale = %.3e" % (mode, tag, int((d != 0).sum()), d.size, worst)
    print(msg)
    if mode == "exact":
        assert np.array_equal(got, want), msg
    else:
        assert (d <= RTOL * scale).all(), msg


TILE_CASES = [((130, 9, 70), p) for p in ("domain", "inside", "low-x-high-z")] + \
             [((65, 5, 33), p) for p in ("domain", "inside", "low-x-high-z")] + \
             [(n, "domain") for n in ((64, 4, 32), (63, 3, 31), (1, 1, 1), (1, 1, 40), (200, 2, 2))]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,placement", TILE_CASES, ids=["%dx%dx%d-%s" % (n + (p,)) for n, p in TILE_CASES])
def test_term_tile_geometry(mode, n, placement):
    """castro_amd_temp_diffusion_fab, source and bare term in one call: several tiles and a ragged last tile in every direction,
    exactly one tile, one zone over and under, minimal boxes, a lone column across a chunk seam; the box as the domain, strictly
    inside it, and on two of its faces.  27 blocks put 24 through the XCD renumbering (3 per XCD) and leave a tail of 3."""
    import torch
    import castro_amd
    rng = np.random.default_rng(1000 * n[0] + 10 * n[2] + len(placement))
    lo, hi, geom = _placed(n, placement)
    diff = _diff()
    U, box = R.ghosted_state(rng, lo, hi, 2, geom)
    v = R.region(box, lo, hi)
    _assert_density_shares(U[R.URHO][v])
    ghosts = np.ones(U.shape[1:], dtype=bool)
    ghosts[v] = False
    if placement == "inside":
        assert np.isfinite(U).all()
    else:
        assert np.isnan(U[R.UTEMP][ghosts]).any() and np.isfinite(U[:, ~ghosts]).all()
    if n == (130, 9, 70):
        assert _blocks(n) == 27
    D, A = R.diffusion_term(U, box, lo, hi, geom, diff)
    assert np.isfinite(D).all() and (n == (1, 1, 1) or (A > 0.0).mean() > 0.9)
    mult = -0.5
    sbox, tbox = R.grow(lo, hi, 3), R.grow(lo, hi, 1)
    sv, tv = R.region(sbox, lo, hi), R.region(tbox, lo, hi)
    src = rng.uniform(-1.0, 1.0, size=(7,) + R.shape_of(sbox))
    term = np.full((1,) + R.shape_of(tbox), -7.0)
    h = castro_amd.HipHydro(0, numerics=mode)
    s, t = _dev(src), _dev(term)
    h.temp_diffusion(_dev(U), box, s, sbox, lo, hi, diff, geom, mult, diff_term=t, diff_term_box=tbox)
    torch.cuda.synchronize()
    assert h.status() == 0
    got, gotD = s.cpu().numpy(), t.cpu().numpy()
    h.close()
    # nothing outside [lo, hi], no other component
    keep = np.ones(src.shape, dtype=bool)
    keep[R.UEDEN][sv] = keep[R.UEINT][sv] = False
    assert np.array_equal(got[keep], src[keep]), "source: a zone outside [lo, hi] or another component was written"
    keep = np.ones(term.shape, dtype=bool)
    keep[0][tv] = False
    assert np.array_equal(gotD[keep], term[keep]), "diff_term: a zone outside [lo, hi] was written"
    # the k-chunk seam first, so that a failure names it: the last plane of a chunk and the first of the next
    for c in range(1, (n[2] + TILE[2] - 1) // TILE[2]):
        for kk in (c * TILE[2] - 1, c * TILE[2]):
            _compare(mode, gotD[0][tv][kk], D[kk], A[kk], "%s %s k-chunk seam, plane lo + %d, bare term" % (n, placement, kk))
    _compare(mode, gotD[0][tv], D, A, "%s %s bare term" % (n, placement))
    for m in (R.UEDEN, R.UEINT):
        _compare(mode, got[m][sv], src[m][sv] + mult * D, np.abs(src[m][sv]) + abs(mult) * A, "%s %s source comp %d" % (n, placement, m))


# five boxes of one periodic-x, outflow-y, wall-z domain of 130 x 40 x 70 zones: (offset from DOMLO, extent, ghost width of the
# state FAB, ghost width of the source FAB)
LEVEL_N = (130, 40, 70)
LEVEL_BOXES = [((0, 0, 0), (130, 9, 70), 2, 3), ((0, 39, 0), (1, 1, 1), 1, 0), ((0, 9, 0), (64, 4, 32), 3, 1),
               ((123, 9, 37), (7, 13, 33), 1, 2), ((64, 13, 20), (40, 24, 16), 2, 3)]


@pytest.mark.parametrize("mode", MODES)
def test_term_many_separate_fabs_in_one_launch(mode):
    """castro_amd_temp_diffusion_mf with five boxes of unequal sizes, each with its own state and source tensors and its own ghost
    widths, cut from one domain so that every ghost zone holds its neighbour's data, the periodic image or a NaN behind a wall;
    the big box first and last in the table (the binary search over start[] at both ends); 43 blocks = 40 renumbered + 3."""
    import torch
    import castro_amd
    rng = np.random.default_rng(4243)
    domhi = tuple(DOMLO[d] + LEVEL_N[d] - 1 for d in range(3))
    geom = _geom(LEVEL_N, DOMLO, lo_bc=(0, 2, 4), hi_bc=(0, 2, 4))
    diff = _diff()
    full, fbox = R.ghosted_state(rng, DOMLO, domhi, 3, geom)
    cover = np.zeros(R.shape_of((DOMLO, domhi)), dtype=int)
    boxes = []
    for off, n, g, gs in LEVEL_BOXES:
        lo = tuple(DOMLO[d] + off[d] for d in range(3))
        hi = tuple(lo[d] + n[d] - 1 for d in range(3))
        cover[R.region((DOMLO, domhi), lo, hi)] += 1
        box, sbox = R.grow(lo, hi, g), R.grow(lo, hi, gs)
        U = np.ascontiguousarray(full[(slice(None),) + R.region(fbox, *box)])
        D, A = R.diffusion_term(U, box, lo, hi, geom, diff)
        assert np.isfinite(D).all()
        boxes.append(dict(lo=lo, hi=hi, box=box, sbox=sbox, U=U, D=D, A=A, src=rng.uniform(-1.0, 1.0, size=(7,) + R.shape_of(sbox))))
    assert cover.max() == 1
    nblocks = sum(_blocks(n) for _, n, _, _ in LEVEL_BOXES)
    assert nblocks == 43 and nblocks % 8 != 0 and (nblocks & ~7) >> 3 > 1
    _assert_density_shares(boxes[0]["U"][R.URHO][R.region(boxes[0]["box"], boxes[0]["lo"], boxes[0]["hi"])])
    mult = -0.5
    h = castro_amd.HipHydro(0, numerics=mode)
    for b in boxes:
        b["Ud"] = _dev(b["U"])
        b["one"] = _dev(b["src"])
        h.temp_diffusion(b["Ud"], b["box"], b["one"], b["sbox"], b["lo"], b["hi"], diff, geom, mult)
    torch.cuda.synchronize()
    for order in ((0, 1, 2, 3, 4), (1, 2, 3, 4, 0)):
        many = {i: _dev(boxes[i]["src"]) for i in order}
        h.temp_diffusion_mf(h.make_diffusion_boxes([(boxes[i]["lo"], boxes[i]["hi"], (boxes[i]["Ud"], boxes[i]["box"]), (many[i], boxes[i]["sbox"]))
                                                    for i in order]), diff, geom, mult)
        torch.cuda.synchronize()
        assert h.status() == 0
        for i in order:
            b = boxes[i]
            tag = "order %s box %d %s" % (order, i, LEVEL_BOXES[i][1])
            assert torch.equal(many[i], b["one"]), tag + ": _mf differs from _fab"               # both builds: bit for bit
            got = many[i].cpu().numpy()
            sv = R.region(b["sbox"], b["lo"], b["hi"])
            keep = np.ones(got.shape, dtype=bool)
            keep[R.UEDEN][sv] = keep[R.UEINT][sv] = False
            assert np.array_equal(got[keep], b["src"][keep]), tag
            for m in (R.UEDEN, R.UEINT):
                _compare(mode, got[m][sv], b["src"][m][sv] + mult * b["D"], np.abs(b["src"][m][sv]) + abs(mult) * b["A"], "%s comp %d" % (tag, m))
    h.close()


# ---- the corrector launch and castro_amd_sources_mf_ex ------------------------------------------------------------------------
STAGE_N = (130, 60, 110)
STAGE_BOXES = [((0, 0, 0), (130, 9, 70)), ((40, 20, 72), (33, 5, 33)), ((129, 59, 109), (1, 1, 1))]
STAGE_DT = 2.e-6                                          # dt * |D| of the size of the state: D ~ k dT / dz^2 ~ 1e5


def _stage_boxes(rng, physical=False):
    """three boxes of a periodic-x domain, each with separate FABs: the big one spans x (the periodic image) and lies on the low
    y and z faces, the second is interior, the single zone sits in the high corner.  S_old and S_new: 2 and 1 ghost zones."""
    from tests.util import physical_state
    domhi = tuple(DOMLO[d] + STAGE_N[d] - 1 for d in range(3))
    geom = _geom(STAGE_N, DOMLO)
    out = []
    for off, n in STAGE_BOXES:
        lo = tuple(DOMLO[d] + off[d] for d in range(3))
        hi = tuple(lo[d] + n[d] - 1 for d in range(3))
        b = dict(lo=lo, hi=hi, n=n, obox=R.grow(lo, hi, 2), nbox=R.grow(lo, hi, 1), sbox=R.grow(lo, hi, 3))
        for key, g in (("So", 2), ("Sn", 1)):
            if physical:                                   # clean_state runs: a thermodynamically consistent state, T varied
                U = physical_state(rng, *R.grow(lo, hi, g), smooth=False)
                U[R.URHO] *= rng.uniform(0.1, 1.0, size=U[R.URHO].shape)
                U[R.UTEMP] = rng.uniform(1.0, 2.0, size=U[R.UTEMP].shape)
            else:
                U = R.random_state(rng, R.shape_of(R.grow(lo, hi, g)))
            b[key] = R.fill_ghosts(U, lo, hi, g, geom)
        v = (slice(None),) + R.region(b["obox"], lo, hi)
        w = (slice(None),) + R.region(b["nbox"], lo, hi)
        assert (b["So"][v] != b["Sn"][w]).all()
        out.append(b)
    return geom, out


def _source_boxes(h, boxes, new, src, sbox, mf=None):
    return h.make_source_boxes([(b["lo"], b["hi"], (b["So_d"], b["obox"]), (b[new], b["nbox"]), (b[src], b[sbox]),
                                 b["mf"] if mf else [None] * 3, b["fb"] if mf else [(b["lo"], b["hi"])] * 3) for b in boxes])


@pytest.mark.parametrize("mode", MODES)
def test_source_stages_with_diffusion_alone(mode):
    """castro_amd_sources_mf_ex with three boxes, grav = rot = NULL, clean_ntimes = 0, against the numpy statement of the two
    stages: the stage-0 launch (init = 1 into a FAB with 3 ghost zones) and the corrector launch (TWO, m1 = 0.5 on S_new,
    m2 = -0.5 on S_old) into a FAB without ghost zones and into one with them.  Every source FAB starts at -7: a kernel that read
    it in place of starting from zero is off by 7, far beyond any tolerance; a ghost zone left alone shows as -7."""
    import torch
    import castro_amd
    P = castro_amd.default_params()
    geom, boxes = _stage_boxes(np.random.default_rng(515))
    diff, dt = _diff(), STAGE_DT
    _assert_density_shares(boxes[0]["So"][R.URHO][R.region(boxes[0]["obox"], boxes[0]["lo"], boxes[0]["hi"])])
    h = castro_amd.HipHydro(0, numerics=mode)
    for b in boxes:
        b["vbox"] = (b["lo"], b["hi"])
        b["So_d"] = _dev(b["So"])
        b["Sn0_d"] = _dev(np.full_like(b["Sn"], 3.25))                                   # stage 0 overwrites the valid zones
        b["Sn1_d"], b["Sn1g_d"] = _dev(b["Sn"]), _dev(b["Sn"])
        b["osrc_d"] = _dev(np.full((7,) + R.shape_of(b["sbox"]), -7.0))
        b["nsrc_d"] = _dev(np.full((7,) + R.shape_of(b["vbox"]), -7.0))
        b["nsrcg_d"] = _dev(np.full((7,) + R.shape_of(b["sbox"]), -7.0))
    h.sources_mf(0, _source_boxes(h, boxes, "Sn0_d", "osrc_d", "sbox"), None, 4, None, geom, P, dt, ntimes=0, diffusion=diff)
    h.sources_mf(1, _source_boxes(h, boxes, "Sn1_d", "nsrc_d", "vbox"), None, 4, None, geom, P, dt, ntimes=0, diffusion=diff)
    h.sources_mf(1, _source_boxes(h, boxes, "Sn1g_d", "nsrcg_d", "sbox"), None, 4, None, geom, P, dt, ntimes=0, diffusion=diff)
    torch.cuda.synchronize()
    assert h.status() == 0
    for nb, b in enumerate(boxes):
        lo, hi = b["lo"], b["hi"]
        runs = [(0, "Sn0_d", "osrc_d", b["sbox"], np.full_like(b["Sn"], 3.25)), (1, "Sn1_d", "nsrc_d", b["vbox"], b["Sn"]),
                (1, "Sn1g_d", "nsrcg_d", b["sbox"], b["Sn"])]
        for stage, new, src, sbox, Sn_in in runs:
            tag = "stage %d box %d %s source FAB %s" % (stage, nb, b["n"], "ghosted" if sbox is b["sbox"] else "valid")
            want_src, want_Sn, A = R.source_stage(stage, b["So"], b["obox"], Sn_in, b["nbox"], sbox, 7, lo, hi, geom, diff, dt)
            got_src, got_Sn = b[src].cpu().numpy(), b[new].cpu().numpy()
            sv = R.region(sbox, lo, hi)
            keep = np.ones(got_src.shape, dtype=bool)
            keep[R.UEDEN][sv] = keep[R.UEINT][sv] = False
            assert not got_src[keep].any(), tag + ": a ghost zone or another component of the source is not zero"
            for m in (R.UEDEN, R.UEINT):
                _compare(mode, got_src[m][sv], want_src[m][sv], A, "%s source comp %d" % (tag, m))
            nv = R.region(b["nbox"], lo, hi)
            base = (b["So"][(slice(None),) + R.region(b["obox"], lo, hi)] if stage == 0 else b["Sn"][(slice(None),) + nv])
            outside = np.ones(got_Sn.shape, dtype=bool)
            outside[(slice(None),) + nv] = False
            assert np.array_equal(got_Sn[outside], Sn_in[outside], equal_nan=True), tag + ": a ghost zone of S_new was written"
            for m in range(8):
                scale = np.abs(base[m]) + (dt * A if m in (R.UEDEN, R.UEINT) else 0.0)
                _compare(mode, got_Sn[m][nv], want_Sn[m][nv], scale, "%s S_new comp %d" % (tag, m))
        # the pieces the corrector launch replaces: two single-term calls into a zeroed FAB, then saxpy
        if mode == "exact":
            z = _dev(np.zeros((7,) + R.shape_of(b["vbox"])))
            Sn2 = _dev(b["Sn"])
            h.temp_diffusion(Sn2, b["nbox"], z, b["vbox"], lo, hi, diff, geom, 0.5)
            h.temp_diffusion(b["So_d"], b["obox"], z, b["vbox"], lo, hi, diff, geom, -0.5)
            h.saxpy(Sn2, b["nbox"], dt, z, b["vbox"], 7, lo, hi)
            torch.cuda.synchronize()
            assert torch.equal(z, b["nsrc_d"]), "box %d: the source of the corrector launch against its pieces" % nb
            assert np.array_equal(Sn2.cpu().numpy(), b["Sn1_d"].cpu().numpy(), equal_nan=True), "box %d: S_new against saxpy" % nb
    h.close()


@pytest.mark.parametrize("mode", MODES)
def test_source_stages_with_diffusion_gravity_and_rotation_equal_the_per_box_calls(mode):
    """the one-launch stages with diffusion, gravity, rotation and clean_state against the per-box sequence temp_diffusion ->
    gravity -> rotation -> apply_source, for the same three boxes with separate FABs: bit for bit in the `exact` build and at
    stage 0 of the `contract` build; the corrector of the `contract` build within the module's tolerance (see below)"""
    import torch
    import castro_amd
    from castro_amd import _lib
    P = castro_amd.default_params(small_dens=0.2)
    rot = castro_amd.make_rotation(3.0, 3, rot_source_type=4)
    grav, gst, dt = (0.3, -0.2, -1.0), 2, STAGE_DT
    diff = _lib.make_diffusion(3.0, 0.1, 0.5, 0.7)                  # the densities of physical_state: across and below this ramp
    h = castro_amd.HipHydro(0, numerics=mode)
    sets = []
    for _ in range(2):
        rng = np.random.default_rng(616)
        geom, boxes = _stage_boxes(rng, physical=True)
        for b in boxes:
            lo, hi = b["lo"], b["hi"]
            b["vbox"] = (lo, hi)
            b["So_d"], b["Sn_d"], b["Sn1_d"] = _dev(b["So"]), _dev(b["Sn"]), _dev(b["Sn"])
            b["osrc_d"] = _dev(np.full((7,) + R.shape_of(b["sbox"]), 9.0))
            b["nsrc_d"] = _dev(np.full((7,) + R.shape_of(b["vbox"]), 9.0))
            b["mf"], b["fb"] = [], []
            for d in range(3):
                fhi = list(hi)
                fhi[d] += 1
                b["fb"].append((lo, tuple(fhi)))
                b["mf"].append(_dev(rng.normal(size=R.shape_of((lo, tuple(fhi))))[None]))
        sets.append(boxes)
    one, lev = sets
    for b in one:
        lo, hi = b["lo"], b["hi"]
        b["osrc_d"].zero_()
        h.temp_diffusion(b["So_d"], b["obox"], b["osrc_d"], b["sbox"], lo, hi, diff, geom, 1.0)
        h.old_gravity_source(b["So_d"], b["obox"], b["osrc_d"], b["sbox"], lo, hi, grav, gst, dt)
        h.old_rotation_source(b["So_d"], b["obox"], b["osrc_d"], b["sbox"], lo, hi, rot, geom, dt)
        h.apply_source(b["Sn_d"], b["nbox"], b["So_d"], b["obox"], dt, b["osrc_d"], b["sbox"], 7, lo, hi, P, ntimes=1)
        b["nsrc_d"].zero_()
        h.temp_diffusion(b["Sn1_d"], b["nbox"], b["nsrc_d"], b["vbox"], lo, hi, diff, geom, 0.5)
        h.temp_diffusion(b["So_d"], b["obox"], b["nsrc_d"], b["vbox"], lo, hi, diff, geom, -0.5)
        h.new_gravity_source(b["So_d"], b["obox"], b["Sn1_d"], b["nbox"], b["nsrc_d"], b["vbox"], b["mf"], b["fb"], lo, hi, grav, gst, dt, geom)
        h.new_rotation_source(b["So_d"], b["obox"], b["Sn1_d"], b["nbox"], b["nsrc_d"], b["vbox"], b["mf"], b["fb"], lo, hi, rot, geom, dt)
        h.apply_source(b["Sn1_d"], b["nbox"], b["Sn1_d"], b["nbox"], dt, b["nsrc_d"], b["vbox"], 7, lo, hi, P, ntimes=1)
    h.sources_mf(0, _source_boxes(h, lev, "Sn_d", "osrc_d", "sbox", mf=True), grav, gst, rot, geom, P, dt, ntimes=1, diffusion=diff)
    h.sources_mf(1, _source_boxes(h, lev, "Sn1_d", "nsrc_d", "vbox", mf=True), grav, gst, rot, geom, P, dt, ntimes=1, diffusion=diff)
    torch.cuda.synchronize()
    assert h.status() == 0
    for nb, (a, b) in enumerate(zip(one, lev)):
        res = {}
        for key in ("osrc_d", "nsrc_d", "Sn_d", "Sn1_d"):
            x, y = a[key].cpu().numpy(), b[key].cpu().numpy()
            d = np.abs(x - y)
            print("%s box %d %s %s: %d of %d values differ, max |delta| = %.3e" % (mode, nb, a["n"], key, int((d > 0).sum()), d.size,
                                                                                 float(np.nanmax(d))))
            res[key] = (x, y, d)
            if mode == "exact" or key in ("osrc_d", "Sn_d"):
                assert np.array_equal(x, y, equal_nan=True), (key, nb, a["n"])
        if mode == "contract":
            # The stage-0 launch equals its pieces bit for bit in this build too.  The corrector does not: between the two
            # single-term calls the sum 0 + 0.5 D(S_new) is rounded and stored, the corrector launch keeps it in a register where
            # the compiler contracts the second half into an FMA (observed on an MI355X: 2881 of 573300 values of the big box,
            # max |delta| 3.6e-12 at |source| ~ 1e5).  So the two energies are held to the module's contract tolerance,
            # |delta| <= RTOL * A with A = 0.5 A(S_new) + 0.5 A(S_old); everything else stays bit for bit.
            lo, hi = a["lo"], a["hi"]
            A = 0.5 * R.diffusion_term(a["Sn"], a["nbox"], lo, hi, geom, diff)[1] + 0.5 * R.diffusion_term(a["So"], a["obox"], lo, hi, geom, diff)[1]
            x, y, d = res["nsrc_d"]
            for m in range(7):
                if m in (R.UEDEN, R.UEINT):
                    assert (d[m] <= RTOL * A).all(), ("nsrc_d", m, nb, float((d[m] / np.maximum(A, 1e-300)).max()))
                else:
                    assert np.array_equal(x[m], y[m]), ("nsrc_d", m, nb)
            # S_new += dt * source, then clean_state: (rho E) and (rho e) carry dt * delta of the source on the scale |base| +
            # dt * A; reset_internal_energy may take (rho e) from (rho E) - kinetic energy, a difference that passes the
            # deviation of (rho E) on unchanged, so (rho e) gets the larger of the two scales; computeTemp is linear in
            # (rho e), T = (rho e) * T / (rho e); density, momenta and species see no diffusion
            x, y, d = res["Sn1_d"]
            nv = R.region(a["nbox"], lo, hi)
            base = a["Sn"][(slice(None),) + nv]
            tol_E = RTOL * (np.abs(base[R.UEDEN]) + dt * A)
            tol_e = RTOL * (np.maximum(np.abs(base[R.UEDEN]), np.abs(base[R.UEINT])) + dt * A)
            tol = {R.UEDEN: tol_E, R.UEINT: tol_e, R.UTEMP: tol_e * np.abs(x[R.UTEMP][nv] / x[R.UEINT][nv])}
            for m in range(8):
                if m in tol:
                    worst = float((d[m][nv] / tol[m]).max()) * RTOL
                    print("contract box %d S_new comp %d: max |delta| / scale = %.3e" % (nb, m, worst))
                    assert (d[m][nv] <= tol[m]).all(), ("Sn1_d", m, nb, worst)
                else:
                    assert np.array_equal(x[m], y[m], equal_nan=True), ("Sn1_d", m, nb)
            outside = np.ones(x.shape, dtype=bool)
            outside[(slice(None),) + nv] = False
            assert np.array_equal(x[outside], y[outside], equal_nan=True)
        v = R.region(a["sbox"], a["lo"], a["hi"])
        osrc, nsrc = a["osrc_d"].cpu().numpy(), a["nsrc_d"].cpu().numpy()
        assert np.isfinite(osrc).all() and np.isfinite(nsrc).all()
        assert np.abs(osrc[R.UEINT][v]).max() > 0 and np.abs(osrc[1][v]).max() > 0 and np.abs(nsrc[R.UEINT]).max() > 0    # diffusion and gravity acted
    h.close()


def test_refused_source_stages_write_nothing():
    """a stage call that is refused has launched nothing: unsupported boundaries (CASTRO_AMD_ERR_UNSUPPORTED) and, at stage 1, an
    S_new without its ghost zone in the LAST box of the table (CASTRO_AMD_ERR_ARG) leave S_new and the source as they were"""
    import torch
    import castro_amd
    from castro_amd import _lib
    P = castro_amd.default_params()
    geom, boxes = _stage_boxes(np.random.default_rng(717))
    diff = _diff()
    h = castro_amd.HipHydro(0)
    for b in boxes:
        b["vbox"] = (b["lo"], b["hi"])
        b["So_d"], b["Sn_d"] = _dev(b["So"]), _dev(b["Sn"])
        b["src"] = np.full((7,) + R.shape_of(b["sbox"]), -7.0)
        b["src_d"] = _dev(b["src"])
    last = boxes[-1]
    last["bare"] = np.ascontiguousarray(last["Sn"][(slice(None),) + R.region(last["nbox"], last["lo"], last["hi"])])
    last["bare_d"] = _dev(last["bare"])

    def call(stage, g, arr):
        return h.lib.castro_amd_sources_mf_ex(h.h, stage, arr[1], arr[0], None, 4, None, C.byref(diff), C.byref(g), C.byref(P), STAGE_DT, 0, None)

    good = _source_boxes(h, boxes, "Sn_d", "src_d", "sbox")
    bad_geom = _geom(STAGE_N, DOMLO, lo_bc=(0, 2, 1), hi_bc=(0, 2, 2))
    for stage in (0, 1):
        assert call(stage, bad_geom, good) == _lib.ERR_UNSUPPORTED
    specs = [(b["lo"], b["hi"], (b["So_d"], b["obox"]), (b["Sn_d"], b["nbox"]), (b["src_d"], b["sbox"]), [None] * 3, [b["vbox"]] * 3) for b in boxes[:-1]]
    specs.append((last["lo"], last["hi"], (last["So_d"], last["obox"]), (last["bare_d"], last["vbox"]), (last["src_d"], last["sbox"]), [None] * 3,
                  [last["vbox"]] * 3))
    assert call(1, geom, h.make_source_boxes(specs)) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert h.status() == 0
    for b in boxes:
        assert np.array_equal(b["Sn_d"].cpu().numpy(), b["Sn"], equal_nan=True) and np.array_equal(b["src_d"].cpu().numpy(), b["src"])
    assert np.array_equal(last["bare_d"].cpu().numpy(), last["bare"])
    # the same table is accepted at stage 0, which reads S_old alone through the stencil
    assert call(0, geom, h.make_source_boxes(specs)) == _lib.OK
    torch.cuda.synchronize()
    assert not np.array_equal(last["bare_d"].cpu().numpy(), last["bare"])
    h.close()


# ---- k_estdt_temp_diffusion ---------------------------------------------------------------------------------------------------
def _estdt_state(rng, box):
    """X = 1 everywhere, so that the limit of a zone is proportional to its density: densities in (1, 2), a fifth of them below
    the cutoff of 0.5"""
    shp = R.shape_of(box)
    U = rng.uniform(0.5, 3.5, size=(8,) + shp)
    rho = rng.uniform(1.0, 2.0, size=shp)
    rho = np.where(rng.uniform(size=shp) < 0.2, 0.3, rho)
    U[R.URHO], U[R.UFS] = rho, rho
    return U


def _estdt(h, mode, U, box, lo, hi, geom, P, diff, max_dt, want, tag, bitwise=False):
    import torch
    out = torch.full((1,), 1.e300, dtype=torch.float64, device="cuda")
    h.estdt_temp_diffusion(_dev(U), box, lo, hi, geom, P, diff, max_dt, out)
    got = out.item()
    print("%s estdt_temp_diffusion %s: %.17g (numpy %.17g)" % (mode, tag, got, want))
    if mode == "exact" or bitwise:
        assert got == want, tag
    else:
        assert abs(got - want) <= RTOL * want, tag
    return got


@pytest.mark.parametrize("mode", MODES)
def test_estdt_temp_diffusion_grid_stride(mode):
    """96 x 96 x 64 = 589 824 zones against a grid capped at 2048 x 256 = 524 288 threads: the smallest density above the cutoff
    lies in the last k-plane, beyond the reach of a kernel that does not stride; the second smallest in the first plane"""
    import castro_amd
    from castro_amd import _lib
    rng = np.random.default_rng(96)
    n = (96, 96, 64)
    lo = DOMLO
    hi = tuple(lo[d] + n[d] - 1 for d in range(3))
    U = _estdt_state(rng, (lo, hi))
    assert n[0] * n[1] * n[2] > 2048 * 256
    for (k, j, i), rho in (((63, 90, 77), 0.6), ((0, 5, 11), 0.7)):
        U[R.URHO][k, j, i] = U[R.UFS][k, j, i] = rho
    assert (63 * 96 + 90) * 96 + 77 >= 2048 * 256
    geom = _geom(n, lo)
    P = _lib.default_params(cfl=0.3)
    diff = _lib.make_diffusion(2.5e7, 0.5)
    want = R.estdt_temp_diffusion(U, (lo, hi), lo, hi, geom, P, diff, 1.e200)
    reach = (hi[0], hi[1], lo[2] + (2048 * 256) // (96 * 96))                        # every plane a single pass touches, the partial one too
    unstrided = R.estdt_temp_diffusion(U, (lo, hi), lo, reach, geom, P, diff, 1.e200)
    assert want < unstrided * (1.0 - 0.1) and unstrided < 1.e100
    h = castro_amd.HipHydro(0, numerics=mode)
    _estdt(h, mode, U, (lo, hi), lo, hi, geom, P, diff, 1.e200, want, "grid stride")
    h.close()


@pytest.mark.parametrize("mode", MODES)
def test_estdt_temp_diffusion_nan_cutoff_ghosts_and_mf(mode):
    import torch
    import castro_amd
    from castro_amd import _lib
    rng = np.random.default_rng(97)
    n = (9, 7, 5)
    lo = DOMLO
    hi = tuple(lo[d] + n[d] - 1 for d in range(3))
    vbox = (lo, hi)
    geom = _geom(n, lo)
    P = _lib.default_params(cfl=0.3)
    diff = _lib.make_diffusion(2.5e7, 0.5)
    below = 5.0 / 0.3
    h = castro_amd.HipHydro(0, numerics=mode)
    # a NaN in UFS of the zone that would set the limit is dropped: the minimum of the others
    U = _estdt_state(rng, vbox)
    U[R.URHO][2, 3, 4], U[R.UFS][2, 3, 4] = 0.6, np.nan
    want = R.estdt_temp_diffusion(U, vbox, lo, hi, geom, P, diff, 5.0)
    V = U.copy()
    V[R.UFS][2, 3, 4] = 0.6
    assert R.estdt_temp_diffusion(V, vbox, lo, hi, geom, P, diff, 5.0) < want < below
    _estdt(h, mode, U, vbox, lo, hi, geom, P, diff, 5.0, want, "NaN in UFS")
    # NaN densities are not above the cutoff, and neither is a density equal to it: max_dt / cfl, in both builds
    for tag, rho in (("NaN in URHO", np.nan), ("rho == cutoff", 0.5)):
        U = _estdt_state(rng, vbox)
        U[R.URHO] = rho
        _estdt(h, mode, U, vbox, lo, hi, geom, P, diff, 5.0, below, tag, bitwise=True)
    # one corner zone above the cutoff
    U = _estdt_state(rng, vbox)
    U[R.URHO] = 0.4
    U[R.URHO][-1, -1, -1] = U[R.UFS][-1, -1, -1] = 0.9
    want = R.estdt_temp_diffusion(U, vbox, lo, hi, geom, P, diff, 5.0)
    assert want < below
    _estdt(h, mode, U, vbox, lo, hi, geom, P, diff, 5.0, want, "a single corner zone above the cutoff")
    # a FAB with 2 ghost zones: the smallest density sits in a ghost zone and is not picked up
    gbox = R.grow(lo, hi, 2)
    U = _estdt_state(rng, gbox)
    U[R.URHO][1, 4, 6] = U[R.UFS][1, 4, 6] = 0.6
    want = R.estdt_temp_diffusion(U, gbox, lo, hi, geom, P, diff, 5.0)
    assert R.estdt_temp_diffusion(U, gbox, gbox[0], gbox[1], geom, P, diff, 5.0) < want * (1.0 - 0.1)
    _estdt(h, mode, U, gbox, lo, hi, geom, P, diff, 5.0, want, "ghosted FAB")
    # three boxes in three FABs: the minimum of the three single-box calls, and numpy's
    specs, wants, outs = [], [], []
    for nb, (nn, g) in enumerate((((9, 7, 5), 2), ((1, 1, 1), 0), ((70, 3, 33), 1))):
        blo = tuple(DOMLO[d] + 20 * nb for d in range(3))
        bhi = tuple(blo[d] + nn[d] - 1 for d in range(3))
        box = R.grow(blo, bhi, g)
        U = _estdt_state(rng, box)
        if nb == 1:
            U[R.URHO] = U[R.UFS] = 0.8
        Ud = _dev(U)
        specs.append((blo, bhi, (Ud, box)))
        wants.append(R.estdt_temp_diffusion(U, box, blo, bhi, geom, P, diff, 5.0))
        out = torch.full((1,), 1.e300, dtype=torch.float64, device="cuda")
        h.estdt_temp_diffusion(Ud, box, blo, bhi, geom, P, diff, 5.0, out)
        outs.append(out.item())
    assert min(wants) == wants[1] and len(set(wants)) == 3                           # the single zone sets the level's limit
    out = torch.full((1,), 1.e300, dtype=torch.float64, device="cuda")
    h.estdt_temp_diffusion_mf(h.make_state_boxes(specs), geom, P, diff, 5.0, out)
    got = out.item()
    print("%s estdt_temp_diffusion_mf: %.17g, single-box calls %s, numpy %.17g" % (mode, got, outs, min(wants)))
    assert got == min(outs)
    if mode == "exact":
        assert got == min(wants)
    else:
        assert abs(got - min(wants)) <= RTOL * min(wants)
    h.close()

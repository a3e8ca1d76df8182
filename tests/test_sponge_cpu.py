"""The sponge (castro.do_sponge) without a GPU: known answers of the numpy restatement (tests/sponge_ref.py), the checks of
make_sponge, and the drivers -- Castro and CastroAmr -- on SpongeOracleBackend, which sends them down the separate-call path."""
import types

import numpy as np
import pytest

from tests import monopole_ref as R
from tests import sponge_ref as S
from castro_amd import _lib


# what a value that went through the ramp's cos may differ by, relatively, from the same expression with another cos (numpy's is
# not glibc's): a few units in the last place of a factor between lower_factor and upper_factor
RAMP_REL = 1e-15


def _geom(n=(4, 4, 4), hi=(4.0, 4.0, 4.0)):
    return _lib.make_geom(n, (0.0, 0.0, 0.0), hi, (2, 2, 2), (2, 2, 2))


def _params():
    return types.SimpleNamespace(eos_gamma=1.4, abar=1.0)


def _state(rho, mom=(1.0, -2.0, 0.5), T=1.0):
    rho = np.asarray(rho, dtype=np.float64)
    U = np.zeros((8,) + rho.shape)
    U[S.URHO] = rho
    for n in range(3):
        U[S.UMX + n] = mom[n]
    U[S.UTEMP], U[S.UFS] = T, rho
    U[S.UEINT] = 1.0
    U[S.UEDEN] = 1.0 + 0.5 * sum(m * m for m in mom) / rho
    return U


def _factor(sp, rad, rho, p):
    a = lambda v: np.array([float(v)])
    return float(S.sponge_factor(sp, a(rad), a(rho), a(p))[0])


def test_factor_below_midpoint_and_above_each_ramp():
    lf, uf = 0.25, 0.75
    mid = lf + 0.5 * (uf - lf)
    sp = _lib.make_sponge(1.0, lower_radius=1.0, upper_radius=3.0, lower_factor=lf, upper_factor=uf, center=(0, 0, 0))
    assert _factor(sp, 0.5, 1.0, 1.0) == lf and _factor(sp, 3.5, 1.0, 1.0) == uf
    assert _factor(sp, 2.0, 1.0, 1.0) == pytest.approx(mid, rel=RAMP_REL)
    assert _factor(sp, 1.0, 1.0, 1.0) == lf and _factor(sp, 3.0, 1.0, 1.0) == pytest.approx(uf, rel=RAMP_REL)
    # density: rho ABOVE the upper density gets the LOWER factor
    sp = _lib.make_sponge(1.0, lower_density=1.0, upper_density=3.0, lower_factor=lf, upper_factor=uf, center=(0, 0, 0))
    assert _factor(sp, 0.0, 3.5, 1.0) == lf and _factor(sp, 0.0, 0.5, 1.0) == uf
    assert _factor(sp, 0.0, 2.0, 1.0) == pytest.approx(mid, rel=RAMP_REL)
    sp = _lib.make_sponge(1.0, lower_pressure=1.0, upper_pressure=3.0, lower_factor=lf, upper_factor=uf, center=(0, 0, 0))
    assert _factor(sp, 0.0, 1.0, 3.5) == lf and _factor(sp, 0.0, 1.0, 0.5) == uf
    assert _factor(sp, 0.0, 1.0, 2.0) == pytest.approx(mid, rel=RAMP_REL)


def test_density_overrides_radius_and_pressure_overrides_both():
    kw = dict(lower_radius=1.0, upper_radius=3.0, lower_factor=0.0, upper_factor=1.0, center=(0, 0, 0))
    r_only = _lib.make_sponge(1.0, **kw)
    assert _factor(r_only, 3.5, 10.0, 10.0) == 1.0
    rd = _lib.make_sponge(1.0, lower_density=1.0, upper_density=3.0, **kw)
    assert _factor(rd, 3.5, 10.0, 10.0) == 0.0                # far out, but dense: the density says lower factor
    assert _factor(rd, 0.5, 0.5, 10.0) == 1.0                 # inside the lower radius, but thin
    rdp = _lib.make_sponge(1.0, lower_density=1.0, upper_density=3.0, lower_pressure=1.0, upper_pressure=3.0, **kw)
    assert _factor(rdp, 3.5, 0.5, 10.0) == 0.0                # radius and density say 1, the pressure says 0
    assert _factor(rdp, 0.5, 10.0, 0.5) == 1.0


def test_a_ramp_left_at_its_default_stays_off():
    sp = _lib.make_sponge(1.0, lower_density=1.0, upper_density=3.0, center=(0, 0, 0))
    assert (sp.lower_radius, sp.upper_radius, sp.lower_pressure, sp.upper_pressure) == (-1.0, -1.0, -1.0, -1.0)
    assert (sp.lower_factor, sp.upper_factor, sp.implicit) == (0.0, 1.0, 1) and list(sp.target_velocity) == [0.0, 0.0, 0.0]
    info = {}
    S.sponge_factor(sp, np.array([0.1, 9.9]), np.array([10.0, 10.0]), np.array([1e-9, 1e9]), info)
    assert set(info["region"]) == {"density"} and np.all(info["factor"] == 0.0)
    # an upper radius alone (lower radius at its default -1) does not make a radial sponge
    sp = _lib.make_sponge(1.0, upper_radius=3.0, lower_density=1.0, center=(0, 0, 0))
    info = {}
    S.sponge_factor(sp, np.array([5.0]), np.array([1.0]), np.array([1.0]), info)
    assert info["region"] == {} and info["factor"][0] == 0.0


def _source(sp, U, dt=0.5, info=None):
    n = U.shape[1:]
    box = ((0, 0, 0), (n[2] - 1, n[1] - 1, n[0] - 1))
    return S.apply_sponge(U, box, box[0], box[1], sp, _geom(), _params(), dt, info)


def test_explicit_against_implicit_and_the_energy_source():
    U = _state(np.full((4, 4, 4), 2.0))
    dt, ts = 0.5, 2.0
    alpha = dt / ts
    kw = dict(lower_density=5.0, upper_density=5.0, center=(0, 0, 0))         # rho = 2 < 5: factor 1 everywhere
    imp, exp = _source(_lib.make_sponge(ts, implicit=1, **kw), U, dt), _source(_lib.make_sponge(ts, implicit=0, **kw), U, dt)
    for n, m in enumerate((1.0, -2.0, 0.5)):
        assert np.all(exp[S.UMX + n] == m * (-alpha * 1.0) / dt)
        assert np.all(imp[S.UMX + n] == m * -(1.0 - 1.0 / (1.0 + alpha)) / dt)
        # the implicit form is the momentum after the update: m + dt Sr = m / (1 + alpha f)
        assert np.allclose(m + dt * imp[S.UMX + n], m / (1.0 + alpha), rtol=1e-15)
    for src in (imp, exp):
        v = [U[S.UMX + n] * (1.0 / U[S.URHO]) for n in range(3)]
        assert np.array_equal(src[S.UEDEN], ((0.0 + v[0] * src[S.UMX]) + v[1] * src[S.UMY]) + v[2] * src[S.UMZ])
        assert np.all(src[S.UEDEN] < 0.0)
        for n in (S.URHO, S.UEINT, S.UTEMP):
            assert np.all(src[n] == 0.0)
    assert imp.shape[0] == S.NSRC


def test_gas_at_the_target_velocity_gets_an_exactly_zero_source():
    rho = np.random.default_rng(3).uniform(0.5, 4.0, size=(4, 4, 4))
    vt = (0.25, -0.5, 2.0)                       # rho * vt is exact only where the product is; U holds the same product
    U = _state(rho)
    for n in range(3):
        U[S.UMX + n] = rho * vt[n]
    sp = _lib.make_sponge(0.1, lower_density=5.0, upper_density=5.0, target_velocity=vt, center=(0, 0, 0))
    src = _source(sp, U)
    assert np.all(src == 0.0)


def test_make_sponge_refuses_what_the_reference_refuses():
    with pytest.raises(ValueError, match="sponge_timescale must be positive"):
        _lib.make_sponge(0.0, lower_radius=1.0, upper_radius=2.0)
    with pytest.raises(ValueError, match="sponge_timescale must be positive"):
        _lib.make_sponge(-1.0, lower_radius=1.0, upper_radius=2.0)
    with pytest.raises(ValueError, match="at least one of the upper radius, density, or pressure"):
        _lib.make_sponge(1.0, lower_radius=1.0)
    with pytest.raises(ValueError, match="at least one of the lower radius, density, or pressure"):
        _lib.make_sponge(1.0, upper_density=1.0)
    sp = _lib.make_sponge(1.e-3, lower_density=1.e-3, upper_density=1.e-3)        # inputs_3d_monopole_regtest
    assert sp.timescale == 1.e-3 and not sp.center_given
    assert _lib.make_sponge(1.0, lower_radius=0.0, upper_radius=1.0, center=(1, 2, 3)).center_given


def test_the_library_exports_the_sponge_entry_points():
    import ctypes as C
    for mode in _lib.NUMERICS_MODES:
        L = _lib.load(mode)
        assert L.castro_amd_new_sponge_source_fab is not None and L.castro_amd_sources_mf_opts is not None
        assert L.castro_amd_abi_version() == 5
    assert C.sizeof(_lib.Sponge) == 15 * 8 + 8                 # twelve reals + center[3] + implicit (+ tail padding)
    assert C.sizeof(_lib.SourceOpts) == 7 * 8


# ---- the drivers ------------------------------------------------------------------------------------------------------------
def _sedov(oracle, n=(16, 16, 16), steps=3, **kw):
    import castro_amd
    c = castro_amd.Castro(n, params=oracle.default_params(init_shrink=0.1), hydro=S.SpongeOracleBackend(), **kw)
    c.initData("sedov", r_init=0.1, nsub=4)
    return c, [c.step() for _ in range(steps)]


def test_a_sponge_alone_takes_the_source_path_and_a_long_timescale_is_no_sponge(oracle):
    free, fdts = _sedov(oracle)
    assert not free.have_sources
    sp = _lib.make_sponge(1.e-2, lower_radius=0.05, upper_radius=0.3)
    c, dts = _sedov(oracle, sponge=sp)
    assert c.have_sources and list(sp.center) == [0.5, 0.5, 0.5]          # the middle of the domain
    src = c.new_source.numpy()
    assert np.abs(src[S.UMX:S.UMZ + 1]).max() > 0.0 and np.abs(src[S.UEDEN]).max() > 0.0
    for n in (S.URHO, S.UEINT, S.UTEMP):
        assert np.all(src[n] == 0.0)
    d = R.field_deviation(c.S_new().numpy(), free.S_new().numpy())
    assert d[S.UMX] > 1e-3, d
    # alpha = dt / 1e30: fac = -(1 - 1 / (1 + 1e-30 f)) is exactly zero, and the source path then only adds zeros
    slow, sdts = _sedov(oracle, sponge=_lib.make_sponge(1.e30, lower_radius=0.05, upper_radius=0.3))
    assert slow.have_sources
    d = R.field_deviation(slow.S_new().numpy(), free.S_new().numpy())
    print("sponge with timescale 1e30 against no sponge: deviation per field", d)
    assert np.all(d <= 1e-12), d
    assert np.allclose(sdts, fdts, rtol=1e-12, atol=0.0)


def test_center_follows_the_driver(oracle):
    import castro_amd
    sp = _lib.make_sponge(1.0, lower_radius=0.1, upper_radius=0.2)
    c = castro_amd.Castro((16, 16, 16), params=oracle.default_params(), hydro=S.SpongeOracleBackend(), sponge=sp)
    c.center = (0.25, 0.5, 0.75)
    assert list(c._sponge_params().center) == [0.25, 0.5, 0.75]
    given = _lib.make_sponge(1.0, lower_radius=0.1, upper_radius=0.2, center=(0.1, 0.2, 0.3))
    c = castro_amd.Castro((16, 16, 16), params=oracle.default_params(), hydro=S.SpongeOracleBackend(), sponge=given)
    c.center = (0.25, 0.5, 0.75)
    assert list(c._sponge_params().center) == [0.1, 0.2, 0.3]


def dust_sponge():
    """castro.do_sponge = 1 of Exec/gravity_tests/DustCollapse/inputs_3d_monopole_regtest"""
    return _lib.make_sponge(1.e-3, lower_density=1.e-3, upper_density=1.e-3)


def test_dust_collapse_sponge_slows_every_moving_ambient_zone(oracle):
    P = oracle.default_params(**R.DUST_PARAMS)
    free, fdts = R.dust_collapse_run(S.SpongeOracleBackend(), P)
    c, dts = R.dust_collapse_run(S.SpongeOracleBackend(), oracle.default_params(**R.DUST_PARAMS), sponge=dust_sponge())
    a, b = c.S_new().numpy(), free.S_new().numpy()
    assert not np.any(a[S.URHO] == 1.e-3) and not np.any(b[S.URHO] == 1.e-3)
    speed = lambda u: np.sqrt(u[S.UMX] ** 2 + u[S.UMY] ** 2 + u[S.UMZ] ** 2) / u[S.URHO]
    amb = (a[S.URHO] < 1.e-3) & (b[S.URHO] < 1.e-3) & (speed(b) > 0.0)
    assert amb.sum() > 100, amb.sum()
    ratio = speed(a)[amb] / speed(b)[amb]
    print("dust collapse, %d moving ambient zones: speed with / without the sponge between %.6g and %.6g (dt = %s)"
          % (amb.sum(), ratio.min(), ratio.max(), dts))
    assert np.all(ratio < 1.0), ratio.max()


class _Recording(S.SpongeOracleBackend):
    """keeps the state every new_sponge_source call was given"""
    calls = None

    def new_sponge_source(self, state_new, new_box, source, src_box, lo, hi, sponge, geom, params, dt, stream=None):
        type(self).calls.append(dict(U=state_new.numpy().copy(), box=new_box, lo=tuple(lo), hi=tuple(hi), dt=float(dt),
                                     dx=tuple(geom.dx[d] for d in range(3)), src=source))
        super().new_sponge_source(state_new, new_box, source, src_box, lo, hi, sponge, geom, params, dt)


def test_amr_every_level_gets_the_sponge_with_its_own_dx(oracle):
    import castro_amd
    _Recording.calls = []
    sp = _lib.make_sponge(1.e-2, lower_radius=0.05, upper_radius=0.3)
    P = oracle.default_params(init_shrink=0.1)
    a = castro_amd.CastroAmr((16, 16, 16), patch_crse=((4, 4, 4), (11, 11, 11)), params=P, make_hydro=_Recording, sponge=sp)
    a.initData("sedov", r_init=0.1, nsub=4)
    a.step()
    for l, lev in enumerate(a.levels):
        assert len(lev.boxes) == 1 and lev.boxes[0].have_sources and lev.boxes[0].sponge is sp
        b = lev.boxes[0]
        mine = [c for c in _Recording.calls if c["src"] is b.new_source]
        assert len(mine) == (1, 2)[l]                   # one coarse step, two fine ones
        last = mine[-1]
        want_dx = tuple(1.0 / (16 * 2 ** l) for _ in range(3))
        assert last["dx"] == want_dx and (last["lo"], last["hi"]) == (b.lo, b.hi)
        geom = _lib.make_geom(tuple(16 * 2 ** l for _ in range(3)), (0., 0., 0.), (1., 1., 1.), (2, 2, 2), (2, 2, 2))
        info = {}
        want = S.apply_sponge(last["U"], last["box"], b.lo, b.hi, sp, geom, P, last["dt"], info)
        got = b.new_source.numpy()
        assert info["cos"].any() and np.abs(want[S.UMX]).max() > 0.0
        assert np.array_equal(got, want), l

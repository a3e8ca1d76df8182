"""The lazy loads of the final stage (LaunchKnobs::lazy_loads, CASTRO_AMD_LAZY_LOADS):

  A. final_flux_tail loads the old state of apply_av only where a face of the pair is compressive (`contract` build);
  B. k_finalx_consup fetches the operands of the evolved (rho e) only where clean_zone keeps it (both builds).

Both branches have to be present in every wave, so the state is cold hypersonic gas in a part of the box: the rough state
of tests/util.physical_state with 300 added to the y velocity in the middle third in x (e / E about 5e-5 < dual_energy_eta2
= 1e-4 there: reset_internal_energy keeps the evolved value), on boxes whose rows (33 and 40 zones) are shorter than a wave,
so that the waves of k_finalx_consup straddle rows and their 63-slot overlap is at work.  One face is a wall.

Bounds: `exact` bit-identical to the oracle (as tests/test_gpu_parity.py), `contract` within rtol 1e-10 measured as
tests/test_gpu_contract.py measures one call (_outputs_deviation); switch on against switch off bit-identical in S_new and the
reductions, fluxes equal as numbers (-0 == +0: a skipped F + (+-0) may leave the other zero).
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.util import physical_state

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SHAPES = [(33, 9, 7), (40, 12, 6)]
DX = (0.02, 0.017, 0.023)
DT = 1.5e-5                                  # cfl 0.3 at |v| + c of about 305 on the shortest zone width
BC = dict(lo_bc=(2, 2, 2), hi_bc=(2, 2, 4))  # outflow, a wall at the high z face
ETA2 = 1.e-4                                 # castro.dual_energy_eta2, the default of both parameter sets


def cold_hypersonic_state(lo, hi, nx_valid, x0):
    """physical_state(rng(7), smooth=False) on [lo, hi] with 300 added to the y velocity in the middle third in x of the valid
    zones (x0: array index of the first valid zone), UEDEN recomputed"""
    U = physical_state(np.random.default_rng(7), lo, hi, smooth=False)
    a, b = x0 + nx_valid // 3, x0 + (2 * nx_valid) // 3
    U[2, :, :, a:b] += 300.0 * U[0, :, :, a:b]
    U[4] = U[5] + 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / U[0]
    return U


def level_state(shape):
    """The initial state of the level drivers: the single call's state, drawn on the box with its ghost zones, cut down to the
    valid zones (27 to 38 % compressive faces).  It is not drawn on the valid zones themselves, because with seed 7 such a draw
    expands nearly everywhere (1 to 2 % compressive faces at 33 x 9 x 7), below what the first test asks for."""
    _, _, sb_lo, sb_hi = _boxes(shape)
    U = cold_hypersonic_state(sb_lo, sb_hi, shape[0], 4)
    return np.ascontiguousarray(U[(slice(None),) + tuple(slice(4, 4 + shape[2 - a]) for a in range(3))])


def kept_mask(S):
    """zones of a cleaned state where reset_internal_energy kept the evolved (rho e): eden - rho ke <= eta2 eden"""
    ke = 0.5 * (S[1] ** 2 + S[2] ** 2 + S[3] ** 2) / S[0]
    return S[4] - ke <= ETA2 * S[4]


def compressive_share(U, dx):
    """numpy restatement of apply_av's face coefficient from an old state U (any box): the share of the faces of each direction,
    among those whose four nodes have all their eight zones inside U, with min(0, average of div(u) at the four nodes) < 0"""
    u, v, w = U[1] / U[0], U[2] / U[0], U[3] / U[0]             # (nz, ny, nx)
    # node (i, j, k) = low corner of zone (i, j, k), from the zones i-1..i, j-1..j, k-1..k: arrays of the nodes 1..n-1
    ux = 0.25 * ((u[1:, 1:, 1:] - u[1:, 1:, :-1]) + (u[:-1, 1:, 1:] - u[:-1, 1:, :-1]) + (u[1:, :-1, 1:] - u[1:, :-1, :-1]) + (u[:-1, :-1, 1:] - u[:-1, :-1, :-1])) / dx[0]
    vy = 0.25 * ((v[1:, 1:, 1:] - v[1:, :-1, 1:]) + (v[:-1, 1:, 1:] - v[:-1, :-1, 1:]) + (v[1:, 1:, :-1] - v[1:, :-1, :-1]) + (v[:-1, 1:, :-1] - v[:-1, :-1, :-1])) / dx[1]
    wz = 0.25 * ((w[1:, 1:, 1:] - w[:-1, 1:, 1:]) + (w[1:, :-1, 1:] - w[:-1, :-1, 1:]) + (w[1:, 1:, :-1] - w[:-1, 1:, :-1]) + (w[1:, :-1, :-1] - w[:-1, :-1, :-1])) / dx[2]
    div = ux + vy + wz                                          # (nz-1, ny-1, nx-1)
    fx = 0.25 * (div[:-1, :-1, :] + div[:-1, 1:, :] + div[1:, :-1, :] + div[1:, 1:, :])      # x face: nodes (j, k), (j+1, k), (j, k+1), (j+1, k+1)
    fy = 0.25 * (div[:-1, :, :-1] + div[:-1, :, 1:] + div[1:, :, :-1] + div[1:, :, 1:])
    fz = 0.25 * (div[:, :-1, :-1] + div[:, :-1, 1:] + div[:, 1:, :-1] + div[:, 1:, 1:])
    return [float((f < 0.0).mean()) for f in (fx, fy, fz)], (fx, fy, fz)


def _boxes(shape):
    bxlo = (0, 0, 0)
    bxhi = tuple(s - 1 for s in shape)
    return bxlo, bxhi, tuple(x - 4 for x in bxlo), tuple(x + 4 for x in bxhi)


def _geoms(oracle, shape):
    import castro_amd
    probhi = [shape[d] * DX[d] for d in range(3)]
    return oracle.make_geom(shape, probhi=probhi, **BC), castro_amd.make_geom(shape, prob_hi=probhi, **BC)


_ORACLE = {}


def oracle_call(oracle, shape):
    """One construct_ctu_hydro_source of the oracle on the box, then min density, clean_state and the CFL estimate twice; computed
    once per shape and shared: {"U", "raw", "S1", "S2", "flux", "mass", "qe", "rmin", "est1", "est2"}"""
    if shape in _ORACLE:
        return _ORACLE[shape]
    bxlo, bxhi, sb_lo, sb_hi = _boxes(shape)
    U = cold_hypersonic_state(sb_lo, sb_hi, shape[0], 4)
    Go, _ = _geoms(oracle, shape)
    Po = oracle.default_params()
    assert Po.dual_energy_eta2 == ETA2
    sl = (slice(None),) + tuple(slice(4, 4 + shape[2 - a]) for a in range(3))
    raw = np.ascontiguousarray(U[sl])
    st, fl, mf, qe = oracle.ctu_hydro(bxlo, bxhi, U, sb_lo, sb_hi, raw, Go, Po, DT, want_qe=True)
    assert st == 0 and np.isfinite(raw).all()
    Lb = oracle.lib()
    S1 = raw.copy()
    rmin = Lb.ora_min_density(oracle.i3(bxlo), oracle.i3(bxhi), oracle.a4(S1, bxlo, bxhi))
    Lb.ora_clean_state(oracle.i3(bxlo), oracle.i3(bxhi), oracle.a4(S1, bxlo, bxhi), C.byref(Po))
    est1 = Lb.ora_estdt_cfl(oracle.i3(bxlo), oracle.i3(bxhi), oracle.a4(S1, bxlo, bxhi), C.byref(Go), C.byref(Po))
    S2 = S1.copy()
    Lb.ora_clean_state(oracle.i3(bxlo), oracle.i3(bxhi), oracle.a4(S2, bxlo, bxhi), C.byref(Po))
    est2 = Lb.ora_estdt_cfl(oracle.i3(bxlo), oracle.i3(bxhi), oracle.a4(S2, bxlo, bxhi), C.byref(Go), C.byref(Po))
    for a in [U, raw, S1, S2] + fl + mf + qe:
        a.setflags(write=False)
    _ORACLE[shape] = dict(U=U, raw=raw, S1=S1, S2=S2, flux=fl, mass=mf, qe=qe, rmin=rmin, est1=est1, est2=est2)
    return _ORACLE[shape]


def _context(numerics, lazy):
    """a context whose knobs were read with CASTRO_AMD_LAZY_LOADS = lazy (None: not set, the default)"""
    from castro_amd.hydro import HipHydro
    old = os.environ.get("CASTRO_AMD_LAZY_LOADS")
    try:
        if lazy is None:
            os.environ.pop("CASTRO_AMD_LAZY_LOADS", None)
        else:
            os.environ["CASTRO_AMD_LAZY_LOADS"] = str(int(lazy))
        h = HipHydro(0, numerics=numerics)
    finally:
        if old is None:
            os.environ.pop("CASTRO_AMD_LAZY_LOADS", None)
        else:
            os.environ["CASTRO_AMD_LAZY_LOADS"] = old
    assert h.numerics == numerics
    return h


def _alloc_outputs(h, U, shape, assign):
    import torch
    bxlo, bxhi, sb_lo, sb_hi = _boxes(shape)
    sl = (slice(None),) + tuple(slice(4, 4 + shape[2 - a]) for a in range(3))
    Ud = torch.from_numpy(np.array(U)).to(h.device)             # copies: the shared arrays are read-only
    Sn = torch.from_numpy(np.array(U[sl])).to(h.device)
    fl, mf, qe, fb = [], [], [], []
    for d in range(3):
        fhi = list(bxhi)
        fhi[d] += 1
        fb.append((bxlo, tuple(fhi)))
        fl.append(h.alloc(8, bxlo, fhi, fill=float("nan") if assign else 0.0))
        mf.append(h.alloc(1, bxlo, fhi))
        qe.append(h.alloc(4, bxlo, fhi))
    return Ud, Sn, fl, mf, qe, fb


def hip_call(h, U, shape, Gh, ntimes, assign):
    """castro_amd_ctu_hydro_clean_fab on the whole box: {"S_new", "flux0..2", "mass0..2", "qe0..2", "red"} as numpy arrays"""
    import torch
    import castro_amd
    bxlo, bxhi, sb_lo, sb_hi = _boxes(shape)
    Ud, Sn, fl, mf, qe, fb = _alloc_outputs(h, U, shape, assign)
    red = torch.full((3,), 1.e200, dtype=torch.float64, device=h.device)
    h.construct_ctu_hydro_source((bxlo, bxhi), Ud, (sb_lo, sb_hi), Sn, (bxlo, bxhi), Gh, castro_amd.default_params(), 0.0, DT,
                                 fluxes=fl, flux_boxes=fb, mass_fluxes=mf, qe=qe, vbx=(bxlo, bxhi), update_from_sborder=True,
                                 clean_ntimes=ntimes, red=red, flux_assign=assign)
    torch.cuda.synchronize()
    out = {"S_new": Sn.cpu().numpy(), "red": red.cpu().numpy()}
    for d in range(3):
        out["flux%d" % d], out["mass%d" % d], out["qe%d" % d] = fl[d].cpu().numpy(), mf[d].cpu().numpy(), qe[d].cpu().numpy()
    return out


def hip_level_call(h, Us, Gh, ntimes, assign):
    """the level-table call (castro_amd_ctu_hydro_mf, one grid per kernel) on the boxes of SHAPES as two boxes of one level"""
    import torch
    import castro_amd
    specs, keep = [], []
    for shape, U in zip(SHAPES, Us):
        bxlo, bxhi, sb_lo, sb_hi = _boxes(shape)
        Ud, Sn, fl, mf, qe, fb = _alloc_outputs(h, U, shape, assign)
        specs.append(((bxlo, bxhi), (bxlo, bxhi), (Ud, (sb_lo, sb_hi)), (Sn, (bxlo, bxhi)), fl, fb, mf))
        keep.append((Sn, fl, mf))
    red = torch.full((3,), 1.e200, dtype=torch.float64, device=h.device)
    h.construct_ctu_hydro_source_mf(None, h.make_hydro_boxes(specs), Gh, castro_amd.default_params(), 0.0, DT, update_from_sborder=True,
                                    flux_assign=assign, clean_ntimes=ntimes, red=red)
    torch.cuda.synchronize()
    assert h.status() == 0
    out = {"red": red.cpu().numpy()}
    for n, (Sn, fl, mf) in enumerate(keep):
        out["S_new_b%d" % n] = Sn.cpu().numpy()
        for d in range(3):
            out["flux%d_b%d" % (d, n)], out["mass%d_b%d" % (d, n)] = fl[d].cpu().numpy(), mf[d].cpu().numpy()
    return out


def _level_run(oracle, shape, flux_assign, numerics):
    """one whole step of the level drivers from the cold hypersonic state: (device driver, oracle level)"""
    import castro_amd
    S0 = level_state(shape)
    probhi = tuple(shape[d] * DX[d] for d in range(3))
    c = castro_amd.Castro(shape, prob_hi=probhi, numerics=numerics, flux_assign=flux_assign, **BC)
    lev = oracle.Level(shape, oracle.make_geom(shape, probhi=probhi, **BC), oracle.default_params(), nthreads=0)
    c.set_state(S0.copy())
    lev.state()[...] = S0
    oracle.lib().ora_level_post_init(lev.h)
    return c, lev, S0


def _both_kinds_in_every_run(kept):
    """every run of 64 zone pairs of every x-row holds zones that keep the evolved (rho e) and zones that reset it"""
    nz, ny, nx = kept.shape
    for a in range(0, nx, 128):
        run = kept[:, :, a:a + 128]
        if not (run.any(axis=2).all() and (~run).any(axis=2).all()):
            return False
    return True


@pytest.mark.parametrize("shape", SHAPES)
def test_both_branches_are_present_in_the_state(oracle, shape):
    """A condition of the tests below, from the oracle's results and the inputs alone: the new state keeps the evolved (rho e) in
    5 to 95 % of the zones and in a part of every 64-pair run of every row, and 3 to 97 % of the faces of each direction are
    compressive -- for the single call and for the whole step of the level driver."""
    o = oracle_call(oracle, shape)
    lev = oracle.Level(shape, oracle.make_geom(shape, probhi=tuple(shape[d] * DX[d] for d in range(3)), **BC), oracle.default_params(), nthreads=0)
    S0 = level_state(shape)
    lev.state()[...] = S0
    oracle.lib().ora_level_post_init(lev.h)
    old = lev.state().copy()
    lev.step()
    new = lev.state().copy()
    assert lev.nretries == 0 and np.isfinite(new).all()
    lev.close()
    for what, Uold, Snew in (("one call", o["U"], o["S1"]), ("level step", old, new)):
        kept = kept_mask(Snew)
        share, _ = compressive_share(Uold, DX)
        print("%s %s: evolved eint kept in %.1f %% of the zones; compressive faces x / y / z: %.1f / %.1f / %.1f %%"
              % (shape, what, 100 * kept.mean(), *[100 * s for s in share]))
        assert 0.05 <= kept.mean() <= 0.95
        assert all(0.03 <= s <= 0.97 for s in share), share
        assert _both_kinds_in_every_run(kept)


def _deviation(got, want):
    from tests.test_gpu_contract import _outputs_deviation
    return _outputs_deviation({k: (got[k], want[k]) for k in want})


def _check_against_oracle(numerics, got, want, what):
    for k in want:
        assert np.isfinite(got[k]).all(), (what, k)
    if numerics == "exact":
        bad = [k for k in want if not np.array_equal(got[k], want[k])]
        assert not bad, "%s not bit-exact: %s" % (what, bad)
    else:
        dev = _deviation(got, want)
        worst = max(dev, key=dev.get)
        print("contract vs oracle, %s: max deviation %.2e (%s)" % (what, dev[worst], worst))
        assert all(v <= RTOL for v in dev.values()), (what, dev)


@pytest.mark.parametrize("numerics", ["exact", "contract"])
@pytest.mark.parametrize("assign", [True, False], ids=["assign", "accumulate"])
@pytest.mark.parametrize("ntimes", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_hydro_call_against_the_oracle(oracle, shape, ntimes, assign, numerics):
    """Every output of one fused call (update, clean_state x ntimes, the reductions) with the lazy loads on: the three flux arrays,
    the mass fluxes, the Godunov states, S_new and the reductions behind dt."""
    o = oracle_call(oracle, shape)
    _, Gh = _geoms(oracle, shape)
    h = _context(numerics, None)
    got = hip_call(h, o["U"], shape, Gh, ntimes, assign)
    assert h.status() == 0
    h.close()
    want = {"S_new": o["S1"] if ntimes == 1 else o["S2"]}
    for d in range(3):
        want["flux%d" % d], want["mass%d" % d], want["qe%d" % d] = o["flux"][d], o["mass"][d], o["qe"][d]
    _check_against_oracle(numerics, got, want, "one call %s x%d %s" % (shape, ntimes, "assign" if assign else "accumulate"))
    red = np.array([o["est1"] if ntimes == 1 else o["est2"], o["rmin"], o["est1"]])
    if numerics == "exact":
        assert got["red"].tolist() == red.tolist()
    else:
        assert np.all(np.abs(got["red"] - red) <= RTOL * np.abs(red)), (got["red"], red)


@pytest.mark.parametrize("numerics", ["exact", "contract"])
@pytest.mark.parametrize("flux_assign", [True, False], ids=["assign", "accumulate"])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_whole_step_against_the_oracle(oracle, shape, flux_assign, numerics):
    """One step of the level driver (the fused update with clean_state twice: ntimes = 2) against the oracle's: S_new, the flux
    registers, the mass fluxes and the next dt."""
    import torch
    c, lev, _ = _level_run(oracle, shape, flux_assign, numerics)
    c.step()
    lev.step()
    dts = (c.computeNewDt(c.dt, est=c._next_est), oracle.lib().ora_level_new_dt(lev.h, lev.dt, lev.time, -1.0))
    torch.cuda.synchronize()
    assert lev.nretries == 0
    got = {"S_new": c.S_new().cpu().numpy()}
    want = {"S_new": lev.state().copy()}
    for d in range(3):
        got["flux%d" % d], want["flux%d" % d] = c.fluxes[d].cpu().numpy(), lev.flux(d).copy()
        got["mass%d" % d] = c.mass_fluxes[d].cpu().numpy()
        want["mass%d" % d] = np.ctypeslib.as_array(oracle.lib().ora_level_mass_flux(lev.h, d), shape=got["mass%d" % d].shape).copy()
        assert got["mass%d" % d].shape == (1,) + want["flux%d" % d].shape[1:] and np.abs(want["mass%d" % d]).max() > 0.0
    _check_against_oracle(numerics, got, want, "level step %s %s" % (shape, "assign" if flux_assign else "accumulate"))
    tol = 0.0 if numerics == "exact" else RTOL
    assert abs(c.dt - lev.dt) <= tol * lev.dt and abs(dts[0] - dts[1]) <= tol * dts[1], (c.dt, lev.dt, dts)
    lev.close()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _assert_switch_invisible(on, off, what):
    for k in on:
        if k.startswith("S_new") or k == "red":
            assert _same_bits(on[k], off[k]), (what, k)
        else:
            assert np.array_equal(on[k], off[k]), (what, k)          # -0 == +0


@pytest.mark.parametrize("numerics", ["exact", "contract"])
@pytest.mark.parametrize("ntimes", [1, 2])
def test_switch_on_equals_switch_off(oracle, numerics, ntimes):
    """CASTRO_AMD_LAZY_LOADS = 1 (both lazy loads), 2 (the artificial viscosity's alone) and 3 (the internal energy's alone) against
    0 in one library on the same inputs, the per-box call and the level-table call: S_new and the reductions bit for bit, fluxes
    equal."""
    Us = [oracle_call(oracle, s)["U"] for s in SHAPES]
    outs = {}
    for lazy in (1, 2, 3, 0):
        h = _context(numerics, lazy)
        outs[lazy] = {}
        for assign in (True, False):
            for shape, U in zip(SHAPES, Us):
                outs[lazy][("box", shape, assign)] = hip_call(h, U, shape, _geoms(oracle, shape)[1], ntimes, assign)
            outs[lazy][("level", assign)] = hip_level_call(h, Us, _geoms(oracle, (40, 12, 7))[1], ntimes, assign)    # a domain that holds both
        assert h.status() == 0
        h.close()
    for lazy in (1, 2, 3):
        for k in outs[lazy]:
            assert np.isfinite(outs[lazy][k]["red"]).all()
            _assert_switch_invisible(outs[lazy][k], outs[0][k], (numerics, ntimes, lazy, k))


@pytest.mark.parametrize("numerics", ["exact", "contract"])
def test_a_nan_in_the_old_state_on_a_non_compressive_face_is_not_hidden(oracle, numerics):
    """(rho E) and (rho e) of one old-state zone whose six faces are not compressive are NaN.  div(u) is formed from the velocities
    and stays what it was, so the lazy tail skips the zone's artificial-viscosity term, which is NaN in the reference.  The NaN
    reaches S_new and the reductions (nan_guard: -1e300, the step is rejected) exactly as with the switch off."""
    shape = SHAPES[0]
    o = oracle_call(oracle, shape)
    U = o["U"].copy()
    _, (fx, fy, fz) = compressive_share(U, DX)
    # faces of U's interior nodes: f*[k, j, i] belongs to node-array index (i, j, k) = zone index + 1 of U
    quiet = None
    nz, ny, nx = U.shape[1:]
    for k in range(5, nz - 5):
        for j in range(5, ny - 5):
            for i in range(5, nx - 5):
                # x faces i, i+1 of zone (i, j, k): fx[k-1, j-1, i-1], fx[k-1, j-1, i]; likewise y and z
                six = (fx[k - 1, j - 1, i - 1], fx[k - 1, j - 1, i], fy[k - 1, j - 1, i - 1], fy[k - 1, j, i - 1], fz[k - 1, j - 1, i - 1], fz[k, j - 1, i - 1])
                if min(six) > 1.0:          # far from zero: a rounding of the restatement cannot change the sign
                    quiet = (k, j, i)
                    break
            if quiet:
                break
        if quiet:
            break
    assert quiet is not None, "no zone with six clearly expanding faces in the state"
    k, j, i = quiet
    U[4, k, j, i] = U[5, k, j, i] = float("nan")
    _, Gh = _geoms(oracle, shape)
    outs = {}
    for lazy in (1, 0):
        h = _context(numerics, lazy)
        outs[lazy] = hip_call(h, U, shape, Gh, 1, True)
        h.close()
    on, off = outs[1], outs[0]
    for o_ in (on, off):
        rejected = bool((o_["red"] == -1.e300).any())                   # nan_guard: a NaN in the density or the CFL estimate
        assert rejected or np.isnan(o_["S_new"]).any(), o_["red"]
    print("NaN zones in S_new: %d (on) %d (off); reductions %s (on) %s (off)"
          % (np.isnan(on["S_new"]).any(axis=0).sum(), np.isnan(off["S_new"]).any(axis=0).sum(), on["red"], off["red"]))
    assert np.array_equal(np.isnan(on["S_new"]), np.isnan(off["S_new"]))
    assert _same_bits(np.nan_to_num(on["S_new"], nan=0.0), np.nan_to_num(off["S_new"], nan=0.0))
    assert _same_bits(on["red"], off["red"])

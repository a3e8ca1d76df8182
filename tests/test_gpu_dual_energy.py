"""The kept-(rho e) branch of reset_internal_energy in every form of the final stage and every clean_state entry point.

Where E - rho ke <= eta2 E, clean_state KEEPS the evolved (rho e) and only floors it at rho small_e.  A fused final stage has to
produce that value (k_finalx_consup fetches its operands lazily, by hand-written offsets, only where it is kept); a zone that
takes the other branch throws it away unseen.  The cases of tests/dual_energy_cases.py put kept and reset zones into every wave,
under every option set that selects another instantiation, from geometries in which the kernel's three zone offsets differ, and
with the update added in place to an S_new that is not Sborder; tests/test_dual_energy_cpu.py asserts those conditions on the
oracle alone.

Bounds, none of them new: `exact` bit-identical to the oracle, `contract` within rtol 1e-10 measured by
tests/test_gpu_contract._outputs_deviation; switch on against switch off and level call against per-box call bit-identical
(fluxes of the switch equal as numbers).
"""
import os

import numpy as np
import pytest

from tests import dual_energy_cases as dc
from tests.test_gpu_lazy_loads import _assert_switch_invisible, _check_against_oracle, _context, _deviation, _same_bits

pytestmark = pytest.mark.gpu

NUMERICS = ["exact", "contract"]


def _ids(cases):
    return [c.name for c in cases]


@pytest.fixture(scope="module")
def ctx():
    """contexts by (numerics, CASTRO_AMD_LAZY_LOADS or None), created on first use and shared by the tests of this file"""
    made = {}

    def get(numerics, lazy=None):
        if (numerics, lazy) not in made:
            made[(numerics, lazy)] = _context(numerics, lazy)
        return made[(numerics, lazy)]
    yield get
    for h in made.values():
        h.close()


def _check_reductions(numerics, got, want, what):
    if numerics == "exact":
        assert got.tolist() == want.tolist(), (what, got, want)
    else:
        assert np.all(np.abs(got - want) <= dc.RTOL * np.abs(want)), (what, got, want)


def _against_the_oracle(h, oracle, case, numerics, assign=True):
    o = dc.oracle_case(oracle, case)
    assert o["status"] == 0
    for ntimes in (1, 2):
        got = dc.hip_case(h, oracle, case, ntimes, assign)
        want, red = dc.wanted(o, ntimes)
        what = "%s x%d %s" % (case.name, ntimes, "assign" if assign else "accumulate")
        _check_against_oracle(numerics, got, want, what)
        _check_reductions(numerics, got["red"], red, what)


# ---- a. every case against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("case", dc.CASES, ids=_ids(dc.CASES))
def test_case_against_the_oracle(oracle, ctx, case, numerics):
    """S_new, the three flux arrays, the mass fluxes, the Godunov states and the three reductions of one fused call with clean_state
    once and twice.  The ghost zones of an S_new FAB larger than the box and Sborder itself must come back untouched."""
    _against_the_oracle(ctx(numerics), oracle, case, numerics)


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("name", ["33x9x7-origin0-sborder-default", "33x9x7-shifted-inplace-default", "33x9x7-tiles-inplace-default"])
def test_accumulated_fluxes_against_the_oracle(oracle, ctx, name, numerics):
    _against_the_oracle(ctx(numerics), oracle, dc.BY_NAME[name], numerics, assign=False)


# ---- b. the switch on every instantiation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("case", dc.SWITCH_CASES, ids=_ids(dc.SWITCH_CASES))
def test_lazy_loads_switch_is_invisible(oracle, ctx, case, numerics):
    """CASTRO_AMD_LAZY_LOADS = 1, 2 and 3 against 0 in one library on the same inputs, from the shifted origin: S_new and the
    reductions bit for bit, fluxes equal as numbers."""
    for ntimes in (1, 2):
        off = dc.hip_case(ctx(numerics, 0), oracle, case, ntimes)
        assert np.isfinite(off["red"]).all()
        for lazy in (1, 2, 3):
            on = dc.hip_case(ctx(numerics, lazy), oracle, case, ntimes)
            _assert_switch_invisible(on, off, (case.name, numerics, ntimes, lazy))


# ---- c. the other forms of the final stage ----------------------------------------------------------------------------------------
_KNOBS = ["CASTRO_AMD_" + k for k in ("TILE_ROWS", "TRACE_TILE_ROWS", "FOLD_TILE_ROWS", "FUSED_TILE_ROWS", "WG", "FINAL_WG", "FUSED_WG", "XPAD",
                                      "FUSE_CONSUP", "FOLD_R1", "FOLD_TILE", "FINAL_TILE", "GL_SOURCES", "GL_PLM", "DIVU_IN_TRACE",
                                      "TRACE_ONE_ZONE", "SIDE_STREAM", "LAZY_LOADS")]
_COLD = ["33x9x7-origin0-sborder-default", "33x9x7-shifted-inplace-default", "33x9x7-tiles-inplace-default", "130x4x3-origin0-sborder-default"]
_FORMS = [
    # id, environment, cases, the kernel its profile must name, kernels it must not name, builds
    ("plain-final-and-consup", {"CASTRO_AMD_FUSE_CONSUP": "0"}, _COLD, "k_consup_clean", ("k_finalx_consup", "k_final_tile"), NUMERICS),
    ("one-launch-final-tile", {"CASTRO_AMD_FINAL_TILE": "1"}, _COLD, "k_final_tile", ("k_finalx_consup", "k_consup_clean"), ["contract"]),
    ("padded-rows", {"CASTRO_AMD_XPAD": "12"}, _COLD, "k_finalx_consup", ("k_consup_clean", "k_final_tile"), NUMERICS),
    ("one-wave-workgroups", {"CASTRO_AMD_WG": "64", "CASTRO_AMD_FUSED_WG": "64"}, _COLD, "k_finalx_consup", ("k_consup_clean", "k_final_tile"), NUMERICS),
    ("plm-general-edges", {"CASTRO_AMD_GL_PLM": "0"}, ["33x9x7-origin0-sborder-plm"], "k_finalx_consup", ("k_consup_clean", "k_final_tile"), NUMERICS),
    ("sources-general-edges", {"CASTRO_AMD_GL_SOURCES": "0"}, ["33x9x7-origin0-sborder-default-src"], "k_finalx_consup", ("k_consup_clean", "k_final_tile"), NUMERICS),
    # the option sets that leave the fused final stage by themselves, in the default context
    ("reset-rhoe-and-temp-fix", {}, ["33x9x7-origin0-sborder-trr", "33x9x7-origin0-sborder-tfix"], "k_consup_clean", ("k_finalx_consup", "k_final_tile"), NUMERICS),
]


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("form", _FORMS, ids=[f[0] for f in _FORMS])
def test_other_forms_of_the_final_stage_against_the_oracle(oracle, form, numerics):
    """The forms of the final stage that remain selectable, each in a context of its own, on the cold state against the oracle; the
    context's profile names the kernel the form is there to run."""
    _, env, names, kernel, others, builds = form
    if numerics not in builds:
        # the one-launch form exists in the `contract` build only: in the other the knob must change nothing
        assert kernel == "k_final_tile"
        kernel, others = "k_finalx_consup", ("k_final_tile", "k_consup_clean")
    old = {k: os.environ.get(k) for k in _KNOBS}
    h = None
    try:
        for k in _KNOBS:
            os.environ.pop(k, None)
        h = dc.context(numerics, env)
        h.profile(True)
        for name in names:
            _against_the_oracle(h, oracle, dc.BY_NAME[name], numerics)
        launched = set(h.profile_report())
        print("%s (%s) launched %s" % (form[0], numerics, sorted(launched)))
        assert kernel in launched and not (set(others) & launched), sorted(launched)
    finally:
        if h is not None:
            h.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- d. the level-table call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("ntimes", [1, 2])
@pytest.mark.parametrize("from_sborder", [True, False], ids=["sborder", "inplace"])
def test_level_table_call_against_the_oracle_and_the_per_box_calls(oracle, ctx, from_sborder, ntimes, numerics):
    """castro_amd_ctu_hydro_mf on the two short-row boxes as two boxes of one level: each box against its own oracle call under the
    bounds above, and against the per-box device call bit for bit, the reductions being the minima over the boxes."""
    h, cases = ctx(numerics), dc.level_cases(from_sborder)
    lvl = dc.hip_level_case(h, oracle, cases, ntimes)
    reds, wants = [], []
    for n, c in enumerate(cases):
        box = dc.hip_case(h, oracle, c, ntimes)
        reds.append(box["red"])
        for k in box:
            if not k.startswith("qe") and k != "red":
                assert _same_bits(lvl["%s_b%d" % (k, n)], box[k]), (c.name, k)
        o = dc.oracle_case(oracle, c)
        want, red = dc.wanted(o, ntimes, qe=False)
        wants.append(red)
        _check_against_oracle(numerics, {k: lvl["%s_b%d" % (k, n)] for k in want}, want, "level call, box %s x%d" % (c.name, ntimes))
    assert _same_bits(lvl["red"], np.minimum(*reds))
    _check_reductions(numerics, lvl["red"], np.minimum(*wants), "level call")


# ---- e. every other clean_state entry point on a state that holds all four kinds of zone -------------------------------------------
def _clean_bounds(numerics, got, want, what):
    assert np.isfinite(got).all(), what
    if numerics == "exact":
        assert _same_bits(got, want), "%s not bit-exact: %d entries differ" % (what, int((got != want).sum()))
    else:
        dev = _deviation({"S": got}, {"S": want})["S"]
        print("contract vs oracle, %s: max deviation %.2e" % (what, dev))
        assert dev <= dc.RTOL, (what, dev)


def _clean_boxes():
    glo, ghi = tuple(x - dc.CLEAN_GROW for x in dc.CLEAN_LO), tuple(x + dc.CLEAN_GROW for x in dc.CLEAN_HI)
    return (glo, ghi), dc.CLEAN_LO, dc.CLEAN_HI


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("ntimes", [1, 2])
@pytest.mark.parametrize("state", dc.CLEAN_STATES, ids=[s[0] for s in dc.CLEAN_STATES])
def test_clean_state_entry_points_on_all_four_kinds_of_zone(oracle, ctx, state, ntimes, numerics):
    """castro_amd_clean_state_fab, castro_amd_clean_state_reduce_fab, castro_amd_clean_state_reduce_mf (two boxes) and the clean
    operation of castro_amd_fab_ops on the valid zones of a FAB with two ghost zones, against ora_clean_state / ora_estdt_cfl; the
    ghost zones stay as they were."""
    import torch
    import castro_amd
    from castro_amd import _lib as L
    name, seed, pkw = state
    h = ctx(numerics)
    box, lo, hi = _clean_boxes()
    G, Go = castro_amd.make_geom((64, 16, 16)), oracle.make_geom((64, 16, 16))
    P = castro_amd.default_params(**pkw)
    Us = [dc.four_kinds_state(oracle, box[0], box[1], seed=s, pkw=pkw)[0] for s in (seed, seed + 100)]
    wants = [dc.oracle_cleans(oracle, U, box, lo, hi, Go, pkw=pkw) for U in Us]
    dev = lambda U: torch.from_numpy(U.copy()).to(h.device)
    valid = dc._within((lo, hi), box)

    def check(got, n, what):
        (S1, S2), rmin, est = wants[n]
        want = S1 if ntimes == 1 else S2
        _clean_bounds(numerics, got[valid], want[valid], "%s, %s x%d" % (what, name, ntimes))
        ghost = np.ones(got.shape, dtype=bool)
        ghost[valid] = False
        assert np.array_equal(got[ghost], Us[n][ghost]), what

    def reds(ns):
        return np.array([min(wants[n][2][ntimes - 1] for n in ns), min(wants[n][1] for n in ns), min(wants[n][2][0] for n in ns)])

    a = dev(Us[0])
    h.clean_state(a, box, lo, hi, P, ntimes=ntimes)
    b, red_b = dev(Us[0]), torch.full((3,), 1.e200, dtype=torch.float64, device=h.device)
    h.clean_state_reduce(b, box, lo, hi, G, P, red_b, ntimes=ntimes)
    c, red_c = [dev(U) for U in Us], torch.full((3,), 1.e200, dtype=torch.float64, device=h.device)
    h.clean_state_reduce_mf(h.make_state_boxes([(lo, hi, (t, box)) for t in c]), G, P, red_c, ntimes=ntimes)
    d = [dev(U) for U in Us]
    h.fab_ops(h.make_ops([(L.OP_CLEAN, 0, 8, lo, hi, float(ntimes), 0.0, (t, box), (t, box), None) for t in d]), params=P)
    torch.cuda.synchronize()
    assert h.status() == 0
    check(a.cpu().numpy(), 0, "clean_state_fab")
    check(b.cpu().numpy(), 0, "clean_state_reduce_fab")
    _check_reductions(numerics, red_b.cpu().numpy(), reds([0]), "clean_state_reduce_fab")
    for n in range(2):
        check(c[n].cpu().numpy(), n, "clean_state_reduce_mf box %d" % n)
        check(d[n].cpu().numpy(), n, "fab_ops clean box %d" % n)
    _check_reductions(numerics, red_c.cpu().numpy(), reds([0, 1]), "clean_state_reduce_mf")


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("ntimes", [1, 2])
@pytest.mark.parametrize("state", dc.CLEAN_STATES, ids=[s[0] for s in dc.CLEAN_STATES])
def test_clean_inside_the_ghost_shell_fill(oracle, ctx, state, ntimes, numerics):
    """castro_amd_fillpatch_shell_fab: the interpolation of a coarse four-kinds state into the ghost shell of a fine box and
    clean_state there, against the oracle's interp-then-clean; the valid zones are not touched."""
    import torch
    import castro_amd
    name, seed, pkw = state
    h = ctx(numerics)
    crse, cbox, fine0, fbox, _ = dc.shell_setup(oracle, seed, pkw)
    want = dc.oracle_shell(oracle, seed, pkw)[ntimes]
    cd, fd = torch.from_numpy(crse.copy()).to(h.device), torch.from_numpy(fine0.copy()).to(h.device)
    h.fillpatch_shell(cd, cbox, fd, fbox, dc.SHELL_VLO, dc.SHELL_VHI, dc.SHELL_GROW, castro_amd.default_params(**pkw), ntimes=ntimes)
    torch.cuda.synchronize()
    got, g = fd.cpu().numpy(), dc.SHELL_GROW
    assert np.array_equal(got[:, g:-g, g:-g, g:-g], fine0[:, g:-g, g:-g, g:-g])
    _clean_bounds(numerics, got, want, "fillpatch_shell_fab, %s x%d" % (name, ntimes))


@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("state", dc.CLEAN_STATES, ids=[s[0] for s in dc.CLEAN_STATES])
def test_sborder_clean_inside_the_hydro_call(oracle, ctx, state, numerics):
    """sborder_clean = 2 of castro_amd_ctu_hydro_fab_ex: clean_state twice on every zone of Sborder inside the pass that reads it.
    Sborder as the call leaves it against the oracle's two cleans.  The outputs of the call: `exact` against the oracle's hydro call
    on the cleaned state, bit for bit.  `contract`: a zone that enforce_min_density rewrote has p = small_pres and e = small_ener to the
    bit, and one ulp in (rho e) of the CLEANED state moves S_new of the oracle itself by 6.0e-4 (four-kinds) and 1.0e-3 (speed-limit) of
    their scale (tests/test_dual_energy_cpu.py prints both), so a comparison with the oracle at 1e-10 would prove nothing; the outputs
    are held to the bits of the same context's plain call on the Sborder the first call left."""
    import torch
    import castro_amd
    name, seed, pkw = state
    h = ctx(numerics)
    U, (lo, hi), sb, probhi = dc.sborder_clean_setup(oracle, seed, pkw)
    want, red_w, st = dc.oracle_sborder_clean(oracle, seed, pkw)
    assert st == 0
    G, P = castro_amd.make_geom(dc.SBC_SHAPE, prob_hi=probhi, **dc.BC), castro_amd.default_params(**pkw)

    def call(Ud, sborder_clean):
        Sn = h.alloc(8, lo, hi, fill=float("nan"))
        fl, mf, fb = [], [], []
        for d in range(3):
            fhi = list(hi)
            fhi[d] += 1
            fb.append((lo, tuple(fhi)))
            fl.append(h.alloc(8, lo, fhi, fill=float("nan")))
            mf.append(h.alloc(1, lo, fhi))
        red = torch.full((3,), 1.e200, dtype=torch.float64, device=h.device)
        h.construct_ctu_hydro_source((lo, hi), Ud, sb, Sn, (lo, hi), G, P, 0.0, dc.SBC_DT, fluxes=fl, flux_boxes=fb, mass_fluxes=mf,
                                     update_from_sborder=True, flux_assign=True, clean_ntimes=1, red=red, sborder_clean=sborder_clean)
        torch.cuda.synchronize()
        assert h.status() == 0
        out = {"Sborder": Ud.cpu().numpy(), "S_new": Sn.cpu().numpy(), "red": red.cpu().numpy()}
        for d in range(3):
            out["flux%d" % d], out["mass%d" % d] = fl[d].cpu().numpy(), mf[d].cpu().numpy()
        return out

    Ud = torch.from_numpy(U.copy()).to(h.device)
    got = call(Ud, 2)
    red = got.pop("red")
    if numerics == "exact":
        _check_against_oracle(numerics, got, want, "sborder_clean = 2, %s" % name)
        _check_reductions(numerics, red, red_w, "sborder_clean = 2, %s" % name)
        return
    # the default path of this build reads neither the temperature nor the species of Sborder after the pass (one species, gamma-law gas:
    # the fused update recomputes both), so k_ctoprim neither cleans nor writes those two planes: they are cleaned, or as they came
    cleaned = got["Sborder"].copy()
    for m in (6, 7):
        if _same_bits(cleaned[m], U[m]):
            cleaned[m] = want["Sborder"][m]
    _check_against_oracle(numerics, {"Sborder": cleaned}, {"Sborder": want["Sborder"]}, "sborder_clean = 2, %s" % name)
    again = call(Ud, 0)
    for k in got:
        assert np.isfinite(got[k]).all() and _same_bits(got[k], again[k]), (name, k)
    assert _same_bits(red, again["red"])


# ---- f. one whole step with sources from the cold state ---------------------------------------------------------------------------
@pytest.mark.parametrize("numerics", NUMERICS)
@pytest.mark.parametrize("flux_assign", [True, False], ids=["assign", "accumulate"])
@pytest.mark.parametrize("shape", dc.SHORT)
def test_one_step_with_gravity_and_rotation_against_the_oracle(oracle, shape, flux_assign, numerics):
    """One step of the level driver with constant gravity (const_grav = -1, grav_source_type 4) and rotation (period 5 about z): the
    driver's in-place fused update (update_from_sborder = False), the sources and their cleans.  S_new, the flux registers, the mass
    fluxes and the next dt against the oracle's level driver."""
    import torch
    lev, c = dc.step_with_sources(oracle, shape, dict(numerics=numerics, flux_assign=flux_assign))
    c.step()
    lev.step()
    dts = (c.computeNewDt(c.dt, est=c._next_est), oracle.lib().ora_level_new_dt(lev.h, lev.dt, lev.time, -1.0))
    torch.cuda.synchronize()
    assert lev.nretries == 0
    got, want = {"S_new": c.S_new().cpu().numpy()}, {"S_new": lev.state().copy()}
    for d in range(3):
        got["flux%d" % d], want["flux%d" % d] = c.fluxes[d].cpu().numpy(), lev.flux(d).copy()
        got["mass%d" % d] = c.mass_fluxes[d].cpu().numpy()
        want["mass%d" % d] = np.ctypeslib.as_array(oracle.lib().ora_level_mass_flux(lev.h, d), shape=got["mass%d" % d].shape).copy()
    _check_against_oracle(numerics, got, want, "step with sources %s %s" % (shape, "assign" if flux_assign else "accumulate"))
    tol = 0.0 if numerics == "exact" else dc.RTOL
    assert abs(c.dt - lev.dt) <= tol * lev.dt and abs(dts[0] - dts[1]) <= tol * dts[1], (c.dt, lev.dt, dts)
    lev.close()

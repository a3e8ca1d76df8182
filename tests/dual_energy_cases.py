"""The cold-state cases of tests/test_dual_energy_cpu.py and tests/test_gpu_dual_energy.py, as data plus builders.

reset_internal_energy has two outcomes per zone: where E - rho ke > eta2 E it overwrites (rho e) from the total energy, else it
KEEPS the evolved (rho e) and floors it at rho small_e.  Every case here is one construct_ctu_hydro_source call on the cold
hypersonic state of tests/test_gpu_lazy_loads.py (seed 7, 300 added to v in the middle third in x: e / E about 5e-5 there), so the
kept outcome is taken in a part of every wave of the fused final stage, under every option set that selects another instantiation
of that stage, from a box origin, ghost widths and S_new FAB that make the three zone offsets of the kernel differ, tile by tile,
and with the update added in place to an S_new that is not Sborder.

A case is data (Case); case_inputs builds its arrays, oracle_case the oracle's results (cached per case, read-only, shared by the
CPU and the GPU tests), hip_case / hip_level_case the device's.
"""
import collections
import ctypes as C
import os

import numpy as np

from tests.test_gpu_lazy_loads import BC, DT, DX, cold_hypersonic_state

RTOL = 1e-10                                 # the `contract` bound of tests/test_gpu_contract.py and tests/test_gpu_lazy_loads.py
SHORT = [(33, 9, 7), (40, 12, 6)]            # rows shorter than a wave
LONG = (130, 4, 3)                           # a row longer than the 126 zones of one wave: the lane-63 hand-over inside a row
SENTINEL = -7.0e77                           # the ghost zones of an S_new FAB larger than the box: nothing may write there

OPTION_SETS = collections.OrderedDict([
    ("default", {}),
    ("cg", dict(riemann_solver=1)),
    ("hllc", dict(riemann_solver=2)),
    ("hybrid", dict(hybrid_riemann=1)),
    ("plm", dict(ppm_type=0)),
    ("limdens", dict(limit_fluxes_on_small_dens=1, small_dens=0.05)),
    ("limvel", dict(limit_fluxes_on_large_vel=1, speed_limit=250.0)),       # enforce_speed_limit acts on the zones moving at 300
    ("trr", dict(transverse_reset_rhoe=1)),
    ("tfix", dict(ppm_temp_fix=2)),
    ("eta0.1", dict(dual_energy_eta2=0.1)),
    ("eta1", dict(dual_energy_eta2=1.0)),
    ("eta0", dict(dual_energy_eta2=0.0)),
    ("smallT3e-9", dict(small_temp=3.e-9)),                                 # rho small_e above the evolved value in some kept zones
    ("smallT1e-8", dict(small_temp=1.e-8)),                                 # ... in nearly all of them (at 3e-8 nothing is kept)
])

Case = collections.namedtuple("Case", "name shape geom from_sborder opt pkw src floor dom")
LEVEL_DOMAIN = (40, 12, 7)                   # holds both short-row boxes as two boxes of one level; its wall is the high z face of the first


def _case(shape, geom="origin0", from_sborder=True, opt="default", src=False, floor=False, pkw=None, dom=None):
    """dom: the domain (from the box's low corner on) where it is not the box itself"""
    pkw = dict(OPTION_SETS[opt] if pkw is None else pkw)
    name = "%dx%dx%d-%s-%s-%s%s%s%s" % (shape + (geom, "sborder" if from_sborder else "inplace", opt, "-src" if src else "",
                                                 "-floor" if floor else "", "-in%dx%dx%d" % dom if dom else ""))
    return Case(name, shape, geom, from_sborder, opt, pkw, src, floor, dom)


def level_cases(from_sborder):
    return [_case(shape, from_sborder=from_sborder, dom=LEVEL_DOMAIN) for shape in SHORT]


def _all_cases():
    cases = [_case(SHORT[0], opt=o) for o in OPTION_SETS]                                          # every option set
    cases.append(_case(SHORT[0], opt="default", src=True))                                         # traced old-time sources
    for o in ("default", "cg", "hllc", "limdens"):                                                 # every geometry, both update modes
        for geom in ("origin0", "shifted", "tiles"):
            for fs in (True, False):
                if not (geom == "origin0" and fs):
                    cases.append(_case(SHORT[0], geom, fs, o))
    cases += [c for fs in (True, False) for c in level_cases(fs)]                                  # the boxes of the level-table call
    cases += [_case(LONG, opt="default"), _case(LONG, opt="limdens"), _case(LONG, "shifted", False, "default")]
    for shape in SHORT:                                                                            # the density floor, in place
        for eta in (None, 1.0):
            pkw = dict(small_dens=0.08)
            if eta is not None:
                pkw["dual_energy_eta2"] = eta
            cases.append(_case(shape, "origin0", False, "floor-eta1" if eta else "floor", floor=True, pkw=pkw))
    return cases


CASES = _all_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SWITCH_CASES = [_case(SHORT[0], "shifted", fs, o) for o in OPTION_SETS for fs in (True, False)] \
    + [_case(SHORT[0], "shifted", fs, "default", src=True) for fs in (True, False)]


def eta2_of(case):
    return case.pkw.get("dual_energy_eta2", 1.e-4)


def boxes(case):
    """{"bx", "sb", "sn": (lo, hi) of the box, of Sborder's FAB and of S_new's FAB; "tiles": the boxes of the device calls}"""
    if case.geom == "shifted":
        lo, sg, ng = (2, -3, 1), (4, 5, 6), (1, 2, 0)
    else:
        lo, sg, ng = (0, 0, 0), (4, 4, 4), (0, 0, 0)
    hi = tuple(lo[d] + case.shape[d] - 1 for d in range(3))
    b = dict(bx=(lo, hi), sb=(tuple(lo[d] - sg[d] for d in range(3)), tuple(hi[d] + sg[d] for d in range(3))),
             sn=(tuple(lo[d] - ng[d] for d in range(3)), tuple(hi[d] + ng[d] for d in range(3))), tiles=[(lo, hi)])
    if case.geom == "tiles":            # a cut at an odd x index (a zone pair straddles the seam) and a cut in y
        xc, yc = lo[0] + ((case.shape[0] // 2) | 1), lo[1] + case.shape[1] // 2
        assert xc % 2 == 1
        b["tiles"] = [(lo, (xc - 1, hi[1], hi[2])), ((xc, lo[1], lo[2]), (hi[0], yc - 1, hi[2])), ((xc, yc, lo[2]), hi)]
    return b


def _within(inner, outer):
    """slices (component, z, y, x) of the box `inner` in an array on the box `outer`"""
    return (slice(None),) + tuple(slice(inner[0][2 - a] - outer[0][2 - a], inner[1][2 - a] - outer[0][2 - a] + 1) for a in range(3))


def _traced_source(U, sb, src_box, scale=0.3):
    """the old-time source of test_ctu_hydro_with_old_sources (gravity-like momentum and energy terms, small density and (rho e)
    terms), times `scale`, on src_box"""
    rng = np.random.default_rng(33)
    s = _within(src_box, sb)
    rho = U[(0,) + s[1:]]
    src = np.zeros((7,) + rho.shape)
    for d, gd in enumerate((0.3, -9.8, 1.7)):
        src[1 + d] = rho * gd
        src[4] += U[(1 + d,) + s[1:]] * gd
    src[0] = 0.01 * rho * rng.uniform(-1, 1, size=rho.shape)
    src[5] = 0.05 * rng.uniform(-1, 1, size=rho.shape)
    return np.ascontiguousarray(scale * src)


_INPUTS = {}


def case_inputs(case, ulp_seed=None):
    """{"U": Sborder, "S0": S_new before the call on the box, "src", "src_box"}.  ulp_seed: (rho e) of every zone moved by one ulp
    with random signs, (rho E) kept consistent (as tools/fuzz_contract.py does), before anything is derived from the state."""
    key = (case.name, ulp_seed)
    if key in _INPUTS:
        return _INPUTS[key]
    b = boxes(case)
    U = cold_hypersonic_state(b["sb"][0], b["sb"][1], case.shape[0], b["bx"][0][0] - b["sb"][0][0])
    if ulp_seed is not None:
        e0 = U[5].copy()
        U[5] *= 1.0 + 2.2e-16 * np.random.default_rng(ulp_seed).choice([-1.0, 1.0], size=e0.shape)
        U[4] = U[4] - e0 + U[5]
    S0 = np.ascontiguousarray(U[_within(b["bx"], b["sb"])])
    if not case.from_sborder:           # S_new is not Sborder: reading the wrong FAB changes the result
        S0 *= 1.0 + 1.e-3 * np.random.default_rng(11).uniform(-1.0, 1.0, size=S0.shape)
    if case.floor:                      # some zones end below small_dens
        S0[:, np.random.default_rng(11).uniform(size=S0.shape[1:]) < 0.2] *= 0.3
    src = src_box = None
    if case.src:
        src_box = (tuple(x - 3 for x in b["bx"][0]), tuple(x + 3 for x in b["bx"][1]))
        src = _traced_source(U, b["sb"], src_box)
    for a in (U, S0, src):
        if a is not None:
            a.setflags(write=False)
    _INPUTS[key] = dict(U=U, S0=S0, src=src, src_box=src_box)
    return _INPUTS[key]


def geoms(oracle, case):
    import castro_amd
    dom = case.dom or case.shape
    probhi = [dom[d] * DX[d] for d in range(3)]
    lo = boxes(case)["bx"][0]
    return oracle.make_geom(dom, probhi=probhi, domlo=lo, **BC), castro_amd.make_geom(dom, prob_hi=probhi, domlo=lo, **BC)


_ORACLE = {}


def oracle_case(oracle, case, ulp_seed=None):
    """One construct_ctu_hydro_source of the oracle on the whole box, then min density, clean_state and the CFL estimate twice;
    computed once per case and shared: {"status", "raw", "S1", "S2", "flux", "mass", "qe", "rmin", "est1", "est2"}"""
    key = (case.name, ulp_seed)
    if key in _ORACLE:
        return _ORACLE[key]
    b, inp = boxes(case), case_inputs(case, ulp_seed)
    (lo, hi), (sb_lo, sb_hi) = b["bx"], b["sb"]
    Go, Po = geoms(oracle, case)[0], oracle.default_params(**case.pkw)
    raw = inp["S0"].copy()
    st, fl, mf, qe = oracle.ctu_hydro(lo, hi, inp["U"], sb_lo, sb_hi, raw, Go, Po, DT, want_qe=True, src=inp["src"],
                                      src_lo=inp["src_box"][0] if case.src else None, src_hi=inp["src_box"][1] if case.src else None)
    Lb = oracle.lib()
    S1 = raw.copy()
    rmin = Lb.ora_min_density(oracle.i3(lo), oracle.i3(hi), oracle.a4(S1, lo, hi))
    Lb.ora_clean_state(oracle.i3(lo), oracle.i3(hi), oracle.a4(S1, lo, hi), C.byref(Po))
    est1 = Lb.ora_estdt_cfl(oracle.i3(lo), oracle.i3(hi), oracle.a4(S1, lo, hi), C.byref(Go), C.byref(Po))
    S2 = S1.copy()
    Lb.ora_clean_state(oracle.i3(lo), oracle.i3(hi), oracle.a4(S2, lo, hi), C.byref(Po))
    est2 = Lb.ora_estdt_cfl(oracle.i3(lo), oracle.i3(hi), oracle.a4(S2, lo, hi), C.byref(Go), C.byref(Po))
    for a in [raw, S1, S2] + fl + mf + qe:
        a.setflags(write=False)
    _ORACLE[key] = dict(status=st, raw=raw, S1=S1, S2=S2, flux=fl, mass=mf, qe=qe, rmin=rmin, est1=est1, est2=est2)
    return _ORACLE[key]


def wanted(o, ntimes, qe=True):
    """the oracle's results as the dict that tests.test_gpu_lazy_loads._check_against_oracle compares, and the three reductions"""
    want = {"S_new": o["S1"] if ntimes == 1 else o["S2"]}
    for d in range(3):
        want["flux%d" % d], want["mass%d" % d] = o["flux"][d], o["mass"][d]
        if qe:
            want["qe%d" % d] = o["qe"][d]
    return want, np.array([o["est1"] if ntimes == 1 else o["est2"], o["rmin"], o["est1"]])


def kept_zones(o, case):
    """(kept, binding, floored): zones where reset_internal_energy kept the evolved (rho e) in the first clean (the test of
    Castro.cpp:3399 on the cleaned state: the clean changes neither side of it again), those of them where the floor rho small_e
    replaced it, and zones whose raw density was below small_dens (enforce_min_density rewrote them; they count as neither)"""
    S, raw = o["S1"], o["raw"]
    floored = raw[0] < oracle_params_small_dens(case)
    ke = 0.5 * (S[1] ** 2 + S[2] ** 2 + S[3] ** 2) / S[0]
    kept = ~(S[4] - ke > eta2_of(case) * S[4]) & ~floored
    binding = kept & (S[5] != raw[5])
    return kept, binding, floored


def both_kinds_in_every_window(kept, n=126):
    """every n consecutive zones, rows taken one after another, hold kept and reset zones: a wave of the fused final stage owns 63
    zone pairs = 126 zones and goes on into the next row where a row ends"""
    cs = np.concatenate([[0], np.cumsum(kept.ravel())])
    cnt = cs[n:] - cs[:-n]
    return bool(((cnt > 0) & (cnt < n)).all())


def oracle_params_small_dens(case):
    return case.pkw.get("small_dens", 1.e-200)


# ---- the device ------------------------------------------------------------------------------------------------------------------
def context(numerics, env=None):
    """a context whose launch knobs were read with the CASTRO_AMD_* variables of `env` set (a value of None: unset); the
    environment is restored before this returns"""
    from castro_amd.hydro import HipHydro
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        h = HipHydro(0, numerics=numerics)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert h.numerics == numerics
    return h


def _device_arrays(h, case, assign):
    import torch
    b, inp = boxes(case), case_inputs(case)
    Ud = torch.from_numpy(np.array(inp["U"])).to(h.device)            # copies: the shared arrays are read-only
    fab = np.full((8,) + tuple(b["sn"][1][2 - a] - b["sn"][0][2 - a] + 1 for a in range(3)), SENTINEL)
    fab[_within(b["bx"], b["sn"])] = inp["S0"]
    Sn = torch.from_numpy(fab).to(h.device)
    srcd = torch.from_numpy(np.array(inp["src"])).to(h.device) if case.src else None
    fl, mf, qe, fb = [], [], [], []
    for d in range(3):
        fhi = list(b["bx"][1])
        fhi[d] += 1
        fb.append((b["bx"][0], tuple(fhi)))
        fl.append(h.alloc(8, b["bx"][0], fhi, fill=float("nan") if assign else 0.0))
        mf.append(h.alloc(1, b["bx"][0], fhi))
        qe.append(h.alloc(4, b["bx"][0], fhi))
    return Ud, Sn, srcd, fl, mf, qe, fb


def _collect(case, Sn, fl, mf, qe, tag=""):
    b = boxes(case)
    fab = Sn.cpu().numpy()
    out = {"S_new" + tag: np.ascontiguousarray(fab[_within(b["bx"], b["sn"])])}
    ghost = np.ones(fab.shape, dtype=bool)
    ghost[_within(b["bx"], b["sn"])] = False
    assert (fab[ghost] == SENTINEL).all(), "%s: the call wrote to zones of S_new's FAB outside the box" % case.name
    for d in range(3):
        out["flux%d%s" % (d, tag)], out["mass%d%s" % (d, tag)] = fl[d].cpu().numpy(), mf[d].cpu().numpy()
        if qe is not None:
            out["qe%d%s" % (d, tag)] = qe[d].cpu().numpy()
    return out


def hip_case(h, oracle, case, ntimes, assign=True):
    """castro_amd_ctu_hydro_clean_fab on the tiles of the case (vbx = the whole box, one `red` for all): {"S_new" (the box's zones),
    "flux0..2", "mass0..2", "qe0..2", "red"} as numpy arrays"""
    import torch
    import castro_amd
    b, inp = boxes(case), case_inputs(case)
    Ud, Sn, srcd, fl, mf, qe, fb = _device_arrays(h, case, assign)
    red = torch.full((3,), 1.e200, dtype=torch.float64, device=h.device)
    Gh, Ph = geoms(oracle, case)[1], castro_amd.default_params(**case.pkw)
    for tile in b["tiles"]:
        h.construct_ctu_hydro_source(tile, Ud, b["sb"], Sn, b["sn"], Gh, Ph, 0.0, DT, fluxes=fl, flux_boxes=fb, mass_fluxes=mf, qe=qe,
                                     vbx=b["bx"], update_from_sborder=case.from_sborder, src=srcd, src_box=inp["src_box"],
                                     clean_ntimes=ntimes, red=red, flux_assign=assign)
    torch.cuda.synchronize()
    assert h.status() == 0
    assert torch.equal(Ud.cpu(), torch.from_numpy(np.array(inp["U"]))), "%s: the call changed Sborder" % case.name
    out = _collect(case, Sn, fl, mf, qe)
    out["red"] = red.cpu().numpy()
    return out


def hip_level_case(h, oracle, cases, ntimes, assign=True):
    """the level-table call (castro_amd_ctu_hydro_mf, one grid per kernel) on the boxes of `cases` as the boxes of one level (same
    origin, option set and update mode; the domain holds them all): the arrays of hip_case with "_b<n>" appended, and "red" """
    import torch
    import castro_amd
    assert len({(c.geom, c.from_sborder, c.opt, c.dom) for c in cases}) == 1 and cases[0].dom and not any(c.src for c in cases)
    specs, keep = [], []
    for c in cases:
        b = boxes(c)
        Ud, Sn, _, fl, mf, _, fb = _device_arrays(h, c, assign)
        specs.append((b["bx"], b["bx"], (Ud, b["sb"]), (Sn, b["sn"]), fl, fb, mf))
        keep.append((Sn, fl, mf))
    Gh = geoms(oracle, cases[0])[1]
    red = torch.full((3,), 1.e200, dtype=torch.float64, device=h.device)
    h.construct_ctu_hydro_source_mf(None, h.make_hydro_boxes(specs), Gh, castro_amd.default_params(**cases[0].pkw), 0.0, DT,
                                    update_from_sborder=cases[0].from_sborder, flux_assign=assign, clean_ntimes=ntimes, red=red)
    torch.cuda.synchronize()
    assert h.status() == 0
    out = {"red": red.cpu().numpy()}
    for n, (c, (Sn, fl, mf)) in enumerate(zip(cases, keep)):
        out.update(_collect(c, Sn, fl, mf, None, "_b%d" % n))
    return out


# ---- a state for the clean_state entry points: no hydro call ------------------------------------------------------------------------
CLEAN_PKW = dict(small_temp=3.e-9, small_dens=0.05)
# (name, seed, parameters).  The second clean of the first state changes (rho E) and (rho e) by an ulp in some hundred zones but not the
# zone that sets the CFL estimate (nor with any other of 39 seeds); with a speed limit it changes momenta too, and with seed 2 the
# estimate: the state that tells the reduction after the first clean from the one after the last.  (The limit takes the kinetic energy
# of the cold zones away, so the groups hold for the first state only.)
CLEAN_STATES = [("four-kinds", 5, CLEAN_PKW), ("speed-limit", 2, dict(CLEAN_PKW, speed_limit=100.0))]
CLEAN_LO, CLEAN_HI, CLEAN_GROW = (1, -2, 3), (37, 2, 5), 2                  # 37 x 5 x 3 zones on a FAB with two ghost zones


def small_e_of(oracle, pkw):
    """e(rho, small_temp) of the gamma-law gas (it does not depend on rho), read off the oracle: a zone at rest without energy comes
    out of clean_state with (rho e) = rho small_e"""
    z = np.zeros((8, 1, 1, 1))
    z[0] = z[7] = 1.0
    z[6] = 1.0
    oracle.lib().ora_clean_state(oracle.i3((0, 0, 0)), oracle.i3((0, 0, 0)), oracle.a4(z, (0, 0, 0), (0, 0, 0)), C.byref(oracle.default_params(**pkw)))
    return float(z[5, 0, 0, 0])


def four_kinds_state(oracle, lo, hi, seed=5, pkw=CLEAN_PKW):
    """(U, group) on [lo, hi]: physical_state(smooth=False) with the zones overwritten in four interleaved groups --
    0 reset zones, left as drawn (e / E of order 0.5);
    1 kept zones: (rho e) at least 2 rho small_e, the momenta raised until e / E = 5e-5, then (rho e) times 1.3, so that it is NOT
      E - rho ke;
    2 kept zones whose (rho e) lies below rho small_e;
    3 zones with rho < small_dens."""
    from tests.util import physical_state
    U = physical_state(np.random.default_rng(seed), lo, hi, smooth=False)
    group = (np.arange(U[0].size).reshape(U[0].shape) * 7 // 3) % 4           # runs of one and two zones of a kind along x
    cold = (group == 1) | (group == 2)
    se = small_e_of(oracle, pkw)
    U[5] = np.where(group == 1, np.maximum(U[5], 2.0 * U[0] * se), U[5])        # clear of the floor
    ke = 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / U[0]
    eb = np.where(group == 2, np.maximum(U[5], U[0] * se), U[5])                # the floor value stays below eta2 E too
    f = np.where(cold, np.sqrt((eb / 5.e-5 - eb) / ke), 1.0)
    for m in (1, 2, 3):
        U[m] *= f
    U[4] = U[5] + 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / U[0]
    U[5] = np.where(group == 1, 1.3 * U[5], U[5])
    U[5] = np.where(group == 2, 0.3 * U[0] * se, U[5])
    U[:, group == 3] *= 0.5 * pkw["small_dens"] / U[0][group == 3]
    return np.ascontiguousarray(U), group


def oracle_cleans(oracle, U, box, lo, hi, Go, pkw=CLEAN_PKW):
    """clean_state twice on [lo, hi] of U (on `box`) in the oracle: [state after one, after two], [raw min density, CFL estimate of
    the raw state restricted to [lo, hi] after one clean, after two]"""
    Po, Lb = oracle.default_params(**pkw), oracle.lib()
    S = U.copy()
    rmin = Lb.ora_min_density(oracle.i3(lo), oracle.i3(hi), oracle.a4(S, *box))
    out, est = [], []
    for _ in range(2):
        Lb.ora_clean_state(oracle.i3(lo), oracle.i3(hi), oracle.a4(S, *box), C.byref(Po))
        est.append(Lb.ora_estdt_cfl(oracle.i3(lo), oracle.i3(hi), oracle.a4(S, *box), C.byref(Go), C.byref(Po)))
        out.append(S.copy())
    return out, rmin, est


# ---- one whole step with gravity and rotation from the cold state: the driver's in-place fused update ----------------------------
STEP_CONST_GRAV = -1.0


def step_with_sources(oracle, shape, device=None):
    """(oracle level, device driver or None) set to the cold state of the level drivers, with constant gravity and rotation;
    device: dict(numerics=, flux_assign=)"""
    from tests.test_gpu_lazy_loads import level_state
    S0 = level_state(shape)
    probhi = tuple(shape[d] * DX[d] for d in range(3))
    center = tuple(0.5 * x for x in probhi)
    lev = oracle.Level(shape, oracle.make_geom(shape, probhi=probhi, **BC), oracle.default_params(), nthreads=0)
    lev.set_gravity(STEP_CONST_GRAV, 4)
    lev.set_rotation(oracle.make_rotation(5.0, 3, center=center))
    lev.state()[...] = S0
    oracle.lib().ora_level_post_init(lev.h)
    c = None
    if device is not None:
        import castro_amd
        c = castro_amd.Castro(shape, prob_hi=probhi, do_grav=True, const_grav=STEP_CONST_GRAV, grav_source_type=4,
                              rotation=castro_amd.make_rotation(5.0, 3, center=center), **dict(BC, **device))
        c.set_state(S0.copy())
    return lev, c


SHELL_VLO, SHELL_VHI, SHELL_GROW = (2, 4, 6), (11, 9, 11), 4


def shell_setup(oracle, seed, pkw):
    """the ghost shell of a fine box filled from a coarse four-kinds state: (crse, crse box, fine before, fine box, the six slabs)"""
    vlo, vhi, g = SHELL_VLO, SHELL_VHI, SHELL_GROW
    flo, fhi = tuple(x - g for x in vlo), tuple(x + g for x in vhi)
    clo, chi = tuple(x // 2 - 1 for x in flo), tuple(x // 2 + 1 for x in fhi)
    crse, _ = four_kinds_state(oracle, clo, chi, seed=seed, pkw=pkw)
    fine0 = np.random.default_rng(23).uniform(1.0, 2.0, size=(8,) + tuple(fhi[d] - flo[d] + 1 for d in (2, 1, 0)))
    shell = [((flo[0], flo[1], flo[2]), (fhi[0], fhi[1], vlo[2] - 1)), ((flo[0], flo[1], vhi[2] + 1), (fhi[0], fhi[1], fhi[2])),
             ((flo[0], flo[1], vlo[2]), (fhi[0], vlo[1] - 1, vhi[2])), ((flo[0], vhi[1] + 1, vlo[2]), (fhi[0], fhi[1], vhi[2])),
             ((flo[0], vlo[1], vlo[2]), (vlo[0] - 1, vhi[1], vhi[2])), ((vhi[0] + 1, vlo[1], vlo[2]), (fhi[0], vhi[1], vhi[2]))]
    return crse, (clo, chi), fine0, (flo, fhi), shell


def oracle_shell(oracle, seed, pkw):
    """interp-then-clean in the oracle: the fine FAB after the interpolation alone, after one clean of the slabs and after two"""
    crse, cbox, fine0, fbox, shell = shell_setup(oracle, seed, pkw)
    Po, want, out = oracle.default_params(**pkw), fine0.copy(), []
    for lo, hi in shell:
        oracle.lib().ora_cc_interp(oracle.i3(lo), oracle.i3(hi), oracle.a4(crse, *cbox), oracle.a4(want, *fbox), 8)
    out.append(want.copy())
    for _ in range(2):
        for lo, hi in shell:
            oracle.lib().ora_clean_state(oracle.i3(lo), oracle.i3(hi), oracle.a4(want, *fbox), C.byref(Po))
        out.append(want.copy())
    return out


# sborder_clean of castro_amd_ctu_hydro_fab_ex: the four-kinds state as the Sborder of one hydro call
SBC_SHAPE, SBC_DT = (37, 5, 3), 5.e-6               # cfl about 0.25 at the 700 or so of the fastest cold zones


def sborder_clean_setup(oracle, seed, pkw, ulp_seed=None):
    lo, hi = (0, 0, 0), tuple(x - 1 for x in SBC_SHAPE)
    sb = (tuple(x - 4 for x in lo), tuple(x + 4 for x in hi))
    U, _ = four_kinds_state(oracle, sb[0], sb[1], seed=seed, pkw=pkw)
    if ulp_seed is not None:
        e0 = U[5].copy()
        U[5] *= 1.0 + 2.2e-16 * np.random.default_rng(ulp_seed).choice([-1.0, 1.0], size=e0.shape)
        U[4] = U[4] - e0 + U[5]
    return U, (lo, hi), sb, [SBC_SHAPE[d] * DX[d] for d in range(3)]


def oracle_sborder_clean(oracle, seed, pkw, ulp_seed=None):
    """clean_state twice on every zone of Sborder, then the hydro call and one fused clean: {"Sborder", "S_new", "flux0..2",
    "mass0..2"}, the reductions, the status"""
    U, (lo, hi), sb, probhi = sborder_clean_setup(oracle, seed, pkw, ulp_seed)
    Go, Po, Lb = oracle.make_geom(SBC_SHAPE, probhi=probhi, **BC), oracle.default_params(**pkw), oracle.lib()
    S = U.copy()
    for _ in range(2):
        Lb.ora_clean_state(oracle.i3(sb[0]), oracle.i3(sb[1]), oracle.a4(S, *sb), C.byref(Po))
    Sn = np.ascontiguousarray(S[_within((lo, hi), sb)])
    st, fl, mf, _ = oracle.ctu_hydro(lo, hi, S, sb[0], sb[1], Sn, Go, Po, SBC_DT)
    rmin = Lb.ora_min_density(oracle.i3(lo), oracle.i3(hi), oracle.a4(Sn, lo, hi))
    Lb.ora_clean_state(oracle.i3(lo), oracle.i3(hi), oracle.a4(Sn, lo, hi), C.byref(Po))
    est = Lb.ora_estdt_cfl(oracle.i3(lo), oracle.i3(hi), oracle.a4(Sn, lo, hi), C.byref(Go), C.byref(Po))
    want = {"Sborder": S, "S_new": Sn}
    for d in range(3):
        want["flux%d" % d], want["mass%d" % d] = fl[d], mf[d]
    return want, np.array([est, rmin, est]), st

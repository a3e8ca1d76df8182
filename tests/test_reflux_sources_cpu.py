"""castro.update_sources_after_reflux on AMR levels (CastroAmr(update_sources_after_reflux=True)): the second half of
Castro::reflux (Castro.cpp:2612-2644, 2762-2868) on the CPU oracle backend -- the registers added to the coarse fluxes, the
new-time sources of both levels taken out, evaluated again and applied.  Geometry and helpers: tests/reflux_sources_ref.py."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import reflux_sources_ref as R
from tests.test_driver_cpu import _free_port

# Test 2's bound: the only non-invertible steps between the stored source and its re-evaluation from (S_old, S_new - dt source)
# are one add / subtract of dt x source and a clean of a clean state, i.e. a few ulp of the state (2.2e-16) times the sensitivity
# of the source to it (of order one for gravity, rotation and the sponge): 1e-11 of the largest source component of the level
# leaves four to five decades.  Measured on the oracle backend with the option on: exactly 0 for gravity and rotation, 1.1e-16
# with the sponge (the docstring of test_the_stored_corrector_belongs_to_the_refluxed_state has every figure).
BOUND = 1.e-11


def _params(oracle, **kw):
    kw.setdefault("init_shrink", 0.5)
    return oracle.default_params(**kw)


def _run(oracle, option, steps=1, backend=None, pkw=None, **kw):
    a = R.make_amr(backend or R.RefluxOracleBackend, _params(oracle, **(pkw or {})), option, **kw)
    R.init_state(a)
    dts = [a.step() for _ in range(steps)]
    return a, dts


# ---- 1. the flux update ---------------------------------------------------------------------------------------------------------
class _Recording(R.RefluxOracleBackend):
    """keeps every register as the reflux reads it"""
    seen = None

    def reflux(self, state, state_box, reg, reg_box, lo, hi, dir, side, ncomp, vol, stream=None):
        type(self).seen[(reg_box, dir, side)] = reg.numpy().copy()
        super().reflux(state, state_box, reg, reg_box, lo, hi, dir, side, ncomp, vol)


def _coarse_fine_faces(cov, d, periodic):
    """bool over the faces of direction d of the domain `cov` spans: exactly one of the two zones of the face is covered"""
    ax = 2 - d
    n = cov.shape[ax]
    pad = [(0, 0)] * 3
    pad[ax] = (1, 1)
    c = np.pad(cov, pad, mode="wrap" if periodic else "constant")
    left = np.take(c, range(0, n + 1), axis=ax)            # zone f - 1 of face f
    right = np.take(c, range(1, n + 2), axis=ax)           # zone f
    return left ^ right


def _register_faces(regs, cov, periodic):
    """[(8, faces of direction d) for d]: the registers [(box, d, array)] on the coarse-fine faces of the domain, 0 elsewhere; a
    register face on a periodic boundary is both ends of the domain"""
    nz, ny, nx = cov.shape
    n = (nx, ny, nz)
    out = []
    for d in range(3):
        shape = [nz, ny, nx]
        shape[2 - d] += 1
        Rg = np.zeros([8] + shape)
        for (lo, hi), rd, arr in regs:
            if rd != d:
                continue
            planes = [lo[d]]
            if periodic[d] and lo[d] in (0, n[d]):
                planes = [0, n[d]]
            for f in planes:
                sl = [slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1)]
                sl[2 - d] = slice(f, f + 1)
                Rg[(slice(None),) + tuple(sl)] = arr
        Rg[:, ~_coarse_fine_faces(cov, d, periodic[d])] = 0.0
        out.append(Rg)
    return out


def _box_faces(Rg, p, d):
    (lo, hi) = p.flux_boxes[d]
    return Rg[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]


def test_registers_reach_the_coarse_fluxes_on_coarse_fine_faces_only(oracle):
    """Pure hydro, one coarse step.  S_new of every box is the option-off run's bit for bit (without sources only the fluxes
    change); on every coarse-fine face -- all six orientations, the low x faces of the first fine box in the OTHER coarse box,
    the wrapped high x faces of the second at x = 0 and x = 16 -- the coarse fluxes are coarse flux + register; on the fine-fine
    face x = 12 and everywhere else they are the option-off run's; the mass fluxes are component URHO of the fluxes on the
    whole level."""
    off, dts_off = _run(oracle, False)
    _Recording.seen = {}
    on, dts_on = _run(oracle, True, backend=_Recording)
    assert dts_on == dts_off
    for lo_, ln_ in zip(off.lev, on.lev):
        for x, y in zip(lo_.boxes, ln_.boxes):
            assert np.array_equal(x.S_new().numpy(), y.S_new().numpy())
    assert len(_Recording.seen) == 12
    cov = R.covered(on, 0)
    regs = [(box, d, arr) for (box, d, side), arr in _Recording.seen.items()]
    Rg = _register_faces(regs, cov, on.periodic)
    changed = 0
    for p_off, p_on in zip(off.lev[0].boxes, on.lev[0].boxes):
        assert p_on.bx == p_off.bx
        for d in range(3):
            add = _box_faces(Rg[d], p_on, d)
            cf = _box_faces(_coarse_fine_faces(cov, d, on.periodic[d])[None], p_on, d)[0]
            f_off, f_on = p_off.fluxes[d].numpy(), p_on.fluxes[d].numpy()
            assert np.array_equal(f_on[:, cf], f_off[:, cf] + add[:, cf])
            assert np.array_equal(f_on[:, ~cf], f_off[:, ~cf])
            assert not cf.any() or np.abs(add[:, cf]).max() > 0.0
            changed += int((f_on != f_off).any(axis=0).sum())
            assert np.array_equal(p_on.mass_fluxes[d].numpy()[0], f_on[0])
    # 4 x 4 faces per side.  x: the face on the seam is in both coarse FABs, the wrapped one at either end of the domain;
    # y, z: two boxes x two sides
    assert changed == 16 * (4 + 4 + 4)
    # the fine-fine face received nothing although both registers hold something there
    ff = [arr for (box, d, side), arr in _Recording.seen.items() if d == 0 and box[0][0] == 12]
    assert len(ff) == 2 and all(np.abs(x).max() > 0.0 for x in ff)


# ---- 2.-4. the stored new-time source is the source of the state it was applied to ------------------------------------------------
def _rotation():
    import castro_amd
    return castro_amd.make_rotation(2.0, rot_axis=3, center=(1.0, 0.5, 0.5))


def _sponge():
    from castro_amd import _lib
    return _lib.make_sponge(5.e-2, lower_radius=0.1, upper_radius=0.6, center=(1.0, 0.5, 0.5))


def _monopole_pm():
    import castro_amd
    return dict(do_grav=True, gravity=castro_amd.MonopoleGravity(drdxfac=2, Gconst=1.0, center=(1.0, 0.5, 0.5)), use_point_mass=True,
                point_mass=0.5, bc=R.OPEN)


CASES = {
    "gravity": lambda: dict(do_grav=True, const_grav=-2.0, grav_source_type=4),
    "rotation": lambda: dict(rotation=_rotation()),
    "sponge": lambda: dict(sponge=_sponge(), backend=R.full_backend()),
    "monopole_pointmass": lambda: dict(backend=R.full_backend(), **_monopole_pm()),
}


@pytest.mark.parametrize("case", list(CASES))
def test_the_stored_corrector_belongs_to_the_refluxed_state(oracle, case):
    """After a coarse step with a dense blob crossing the coarse-fine boundary: on the uncovered coarse zones next to the fine
    level, new_source against the new-time source evaluated by the separate backend calls from (S_old, S_new - dt new_source,
    mass fluxes, gravity).  Option on: equal to rounding (BOUND); option off: the stored source was made from the state and the
    mass fluxes the reflux has since replaced, and misses the bound by more than three decades.  Measured (off / on):
    gravity 5.0e-3 / 0, rotation 1.1e-2 / 0, sponge 8.6e-3 / 1.1e-16, monopole + point mass 5.6e-3 / 0."""
    got = {}
    for option in (False, True):
        a, _ = _run(oracle, option, **CASES[case]())
        zones = R.boundary_zones(a, 0)
        # two x sides and four y / z sides of the fine region; on the open domain its high x side is the physical boundary
        assert zones.sum() == (2 if a.periodic[0] else 1) * 16 + 8 * 16
        got[option] = R.corrector_mismatch(a, 0, zones)
        if option:
            assert R.corrector_mismatch(a, 1) <= BOUND  # the fine level too
    print("%s: mismatch off %.3g, on %.3g" % (case, got[False], got[True]))
    assert got[True] <= BOUND
    assert got[False] >= 1.e3 * BOUND


def test_the_coarse_gravity_field_is_still_its_own_at_the_reflux(oracle):
    """Monopole gravity with a point mass: the fine level's two subcycles construct their own gravity at their own times (binning
    the coarse level too) between the coarse advance and its post_timestep.  The re-evaluation of a coarse box reads the grav_old
    and grav_new FABs its advance's new-time stage read, bit for bit: the field is neither rebuilt nor overwritten."""
    class Rec(R.full_backend()):
        seen = []

        def new_gravity_source_gfab(self, state_old, old_box, state_new, new_box, source, src_box, mass_fluxes, flux_boxes, lo, hi,
                                    grav_old, grav_new, grav_box, grav_source_type, dt, geom, stream=None):
            Rec.seen.append((source.data_ptr(), grav_old.numpy().copy(), grav_new.numpy().copy()))
            super().new_gravity_source_gfab(state_old, old_box, state_new, new_box, source, src_box, mass_fluxes, flux_boxes, lo, hi,
                                            grav_old, grav_new, grav_box, grav_source_type, dt, geom)
    a, _ = _run(oracle, True, **dict(_monopole_pm(), backend=Rec))
    for l, n in ((0, 2), (1, 3)):
        for b in a.lev[l].boxes:
            calls = [c for c in Rec.seen if c[0] == b.new_source.data_ptr()]
            assert len(calls) == n
            assert np.array_equal(calls[-1][1], calls[-2][1]) and np.array_equal(calls[-1][2], calls[-2][2])
            assert np.abs(calls[-1][2]).max() > 0.0 and not np.array_equal(calls[-1][1], calls[-1][2])
    fine_first, fine_last = [[c for c in Rec.seen if c[0] == b.new_source.data_ptr()] for b in a.lev[1].boxes][0][::2]
    assert not np.array_equal(fine_first[2], fine_last[2])      # the fine subcycles did construct fields of their own


class _Counting(R.RefluxOracleBackend):
    """counts the removals of a stored source (saxpy with a negative factor) and the new-gravity constructions per source tensor"""
    removed, made = None, None

    def saxpy(self, dst, dst_box, a, src, src_box, ncomp, lo, hi, stream=None):
        if a < 0.0:
            type(self).removed.append((src.data_ptr(), float(a)))
        super().saxpy(dst, dst_box, a, src, src_box, ncomp, lo, hi)

    def new_gravity_source(self, state_old, old_box, state_new, new_box, source, src_box, mass_fluxes, flux_boxes, lo, hi,
                           grav, grav_source_type, dt, geom, stream=None):
        type(self).made.append((source.data_ptr(), float(dt), state_old.numpy().copy()))
        super().new_gravity_source(state_old, old_box, state_new, new_box, source, src_box, mass_fluxes, flux_boxes, lo, hi,
                                   grav, grav_source_type, dt, geom)


def test_the_fine_level_is_evaluated_again_too(oracle):
    """The re-evaluation runs on the fine level as well, finer level first: per coarse step every fine box has its stored source
    removed once (with the fine dt) and constructed three times (two advances + once after the reflux), every coarse box once
    and twice; the fine level passes the consistency check.  Nothing the fine level's zone-local sources read has changed (its
    own state, mass fluxes and gravity), so its S_new and new_source stay within rounding of the option-off run: taking dt x
    source out of a state and putting it back returns the state's bits in all but rare zones, and in this run in every zone.
    Where a level's state does change -- level 1 of three levels, refluxed by level 2 -- it differs from the option-off run:
    test_the_driver_equals_the_composition_written_out."""
    _Counting.removed, _Counting.made = [], []
    kw = dict(do_grav=True, const_grav=-2.0, rotation=_rotation())
    on, dts = _run(oracle, True, backend=_Counting, **kw)
    off, dts_off = _run(oracle, False, **kw)
    assert dts == dts_off
    fine_dt, crse_dt = dts[0] / 2, dts[0]
    order = [p for p, _ in _Counting.removed]
    fine_ptrs = [b.new_source.data_ptr() for b in on.lev[1].boxes]
    crse_ptrs = [b.new_source.data_ptr() for b in on.lev[0].boxes]
    assert order == fine_ptrs + crse_ptrs
    assert [a for _, a in _Counting.removed] == [-fine_dt] * 2 + [-crse_dt] * 2
    for ptrs, n, dt in ((fine_ptrs, 3, fine_dt), (crse_ptrs, 2, crse_dt)):
        for p in ptrs:
            calls = [c for c in _Counting.made if c[0] == p]
            assert len(calls) == n and calls[-1][1] == dt
    for x, y in zip(off.lev[1].boxes, on.lev[1].boxes):
        for u, v in ((x.S_new().numpy(), y.S_new().numpy()), (x.new_source.numpy(), y.new_source.numpy())):
            assert np.abs(u - v).max() <= 1.e-13 * np.abs(u).max()
    assert R.corrector_mismatch(on, 1) <= BOUND


# ---- 5. three levels ----------------------------------------------------------------------------------------------------------------
def _second_half_of_reflux(a, l):
    """Castro::reflux(l, l + 1) behind the flux correction of the state, written out box by box: the registers of level l + 1 onto
    the coarse-fine faces of the fluxes of level l, the mass fluxes from them, then on level l + 1 and on level l: the stored
    source out of S_new, clean_state, do_new_sources."""
    crse, fine = a.lev[l], a.lev[l + 1]
    regs = [(rbox, d, reg.numpy()) for b in fine.boxes for (d, side), (reg, rbox) in b.regs.items()]
    Rg = _register_faces(regs, R.covered(a, l), a.periodic)
    for p in crse.boxes:
        for d in range(3):
            p.fluxes[d] += torch.from_numpy(_box_faces(Rg[d], p, d))
            p.mass_fluxes[d][0] = p.fluxes[d][0]
    for lev in (fine, crse):
        dt = lev.lastDt
        for b in lev.boxes:
            h = b.hydro
            h.saxpy(b.S_new_b, b.gbox, -dt, b.new_source, b.bx, R.NSRC, b.lo, b.hi)
            h.clean_state(b.S_new_b, b.gbox, b.lo, b.hi, b.params, ntimes=1)
            b._source_stage(1, dt)
        lev.invalidate_estimate()


def _written_out(a):
    """an option-off hierarchy that runs _second_half_of_reflux between the reflux and avgDown of every post_timestep"""
    orig = a.avgDown

    def avg_down(l=1):
        _second_half_of_reflux(a, l - 1)
        orig(l)
    a.avgDown = avg_down
    return a


@pytest.mark.parametrize("patches", [[R.FINE], [R.FINE, R.FINER]], ids=["two-levels", "three-levels"])
def test_the_driver_equals_the_composition_written_out(oracle, patches):
    """Option on against an option-off hierarchy whose post_timestep is completed by hand, two coarse steps, gravity and
    rotation: dt sequence, S_new, new_source, fluxes and mass fluxes of every box of every level bit for bit.  Three levels (a
    level-2 box inside a level-1 box): level 1 is evaluated again at each of its own post_timesteps with level 2 and once more at
    level 0's -- three times per coarse step, level 2 twice, level 0 once."""
    kw = dict(do_grav=True, const_grav=-2.0, rotation=_rotation(), patches=patches)
    _Counting.removed, _Counting.made = [], []
    on = R.make_amr(_Counting, _params(oracle), True, **kw)
    man = R.make_amr(R.RefluxOracleBackend, _params(oracle), False, **kw)
    for a in (on, man):
        R.init_state(a)
    _written_out(man)
    for _ in range(2):
        assert on.step() == man.step()
    for l, (x, y) in enumerate(zip(on.lev, man.lev)):
        for bx, by in zip(x.boxes, y.boxes):
            assert np.array_equal(bx.S_new().numpy(), by.S_new().numpy()), l
            assert np.array_equal(bx.new_source.numpy(), by.new_source.numpy()), l
            for d in range(3):
                assert np.array_equal(bx.fluxes[d].numpy(), by.fluxes[d].numpy()), l
                assert np.array_equal(bx.mass_fluxes[d].numpy(), by.mass_fluxes[d].numpy()), l
    if len(on.lev) == 3:                                # level 1 is refluxed by level 2: its state is not the option-off run's
        off = R.make_amr(R.RefluxOracleBackend, _params(oracle), False, **kw)
        R.init_state(off)
        off.step()
        off.step()
        for name in ("S_new", "new_source"):
            assert any(not np.array_equal(u, v) for u, v in zip(R.level_arrays(off, name)[1], R.level_arrays(on, name)[1]))
    per_step = {2: [1, 1], 3: [1, 3, 2]}[len(on.lev)]
    for l, lev in enumerate(on.lev):
        for b in lev.boxes:
            assert sum(1 for p, _ in _Counting.removed if p == b.new_source.data_ptr()) == 2 * per_step[l], l


# ---- 6. a level whose last advance was split by a retry ---------------------------------------------------------------------------
def _reject_last_fine_advance(a, when=2):
    """the first attempt of the `when`-th advance of level 1 is rejected after it has run: retry_advance_ctu halves it"""
    fine = a.lev[1]
    orig, n = fine.do_advance_ctu, [0]

    def do_advance_ctu(time, dt):
        n[0] += 1
        out = orig(time, dt)
        return (False, "forced rejection", None) if n[0] == when else out
    fine.do_advance_ctu = do_advance_ctu


def test_a_retried_level_is_evaluated_with_its_last_subcycle(oracle):
    """The second fine advance of the coarse step is rejected once and ends in two subcycles of dt / 4.  The re-evaluation after
    the reflux uses the LAST subcycle's dt and old state -- the new-gravity call it makes gets the S_old and the dt of the
    new-time stage of that subcycle --, and afterwards S_old of the fine boxes holds the old data of the whole advance again,
    bit for bit those of the option-off run."""
    kw = dict(do_grav=True, const_grav=-2.0, rotation=_rotation())
    runs = {}
    for option in (False, True):
        _Counting.removed, _Counting.made = [], []
        a = R.make_amr(_Counting, _params(oracle), option, **kw)
        R.init_state(a)
        _reject_last_fine_advance(a)
        dt = a.step()
        assert [(lev.nsubcycles, lev.nretries) for lev in a.levels] == [(1, 0), (2, 1)]
        assert a.lev[1].lastDt == pytest.approx(dt / 4, rel=1e-12)
        runs[option] = (a, list(_Counting.made), list(_Counting.removed))
    on, made, removed = runs[True]
    for b in on.lev[1].boxes:
        calls = [c for c in made if c[0] == b.new_source.data_ptr()]
        # first advance, rejected attempt, two subcycles, the re-evaluation
        assert [c[1] for c in calls] == pytest.approx([dt / 2, dt / 2, dt / 4, dt / 4, dt / 4], rel=1e-12)
        assert calls[-1][1] == calls[-2][1] == on.lev[1].lastDt
        assert np.array_equal(calls[-1][2], calls[-2][2])                   # the old state of the last subcycle
        assert not np.array_equal(calls[-1][2], calls[-3][2])               # not the one of the advance
        assert [x for p, x in removed if p == b.new_source.data_ptr()] == [-on.lev[1].lastDt]
    for x, y in zip(runs[False][0].lev[1].boxes, on.lev[1].boxes):
        assert np.array_equal(x.S_old_b.numpy(), y.S_old_b.numpy())
        assert np.array_equal(y.S_old_b.numpy(), [c for c in made if c[0] == y.new_source.data_ptr()][2][2])
    assert R.corrector_mismatch(on, 0, R.boundary_zones(on, 0)) <= BOUND


def test_mass_fluxes_follow_the_fluxes_when_the_coarse_level_was_subcycled(oracle):
    """A rejected coarse advance: its fluxes are the sums over two subcycles, its mass fluxes those of the last one.  With the
    option the mass fluxes leave post_timestep as component URHO of the (corrected) fluxes on the whole level -- a copy, not
    an add (Castro.cpp:2633-2639); without it they stay the last subcycle's."""
    for option in (False, True):
        a = R.make_amr(R.RefluxOracleBackend, _params(oracle), option, do_grav=True, const_grav=-2.0)
        R.init_state(a)
        crse = a.lev[0]
        orig, n = crse.do_advance_ctu, [0]

        def do_advance_ctu(time, dt, orig=orig, n=n):
            n[0] += 1
            out = orig(time, dt)
            return (False, "forced rejection", None) if n[0] == 1 else out
        crse.do_advance_ctu = do_advance_ctu
        a.step()
        assert (crse.nsubcycles, crse.nretries) == (2, 1)
        same = all(np.array_equal(p.mass_fluxes[d].numpy()[0], p.fluxes[d].numpy()[0]) for p in crse.boxes for d in range(3))
        assert same == option


# ---- 7. castro.source_term_predictor = 1 ------------------------------------------------------------------------------------------
def test_the_predictor_of_the_next_step_reads_the_new_corrector(oracle):
    """Two coarse steps with source_term_predictor = 1: the source corrector level 0 makes at the start of the second step is
    2 / dt x the momentum components of the new_source the first step's re-evaluation has left, not of the one its advance made."""
    kw = dict(do_grav=True, const_grav=-2.0, rotation=_rotation(), pkw=dict(source_term_predictor=1))
    off, _ = _run(oracle, False, **kw)
    on, dts = _run(oracle, True, **kw)
    crse = on.lev[0]
    left = [b.new_source.numpy().copy() for b in crse.boxes]
    assert any(not np.array_equal(x, b.new_source.numpy()) for x, b in zip(left, off.lev[0].boxes))
    orig, got = crse.create_source_corrector, []

    def create_source_corrector():
        orig()
        got.append([b.source_corrector.numpy().copy() for b in crse.boxes])
    crse.create_source_corrector = create_source_corrector
    on.step()
    assert len(got) == 1
    g = 3
    for c, ns, b in zip(got[0], left, crse.boxes):
        n = b.n
        want = torch.from_numpy(ns[1:4].copy()).mul_(2.0 / dts[0]).numpy()
        assert np.array_equal(c[1:4, g:g + n[2], g:g + n[1], g:g + n[0]], want)


# ---- 8. the boxes spread over ranks ---------------------------------------------------------------------------------------------
# "seam": one fine box under each coarse box, each owned by the rank that does NOT own the coarse box under it (fine box i on
# rank (i + 1) mod 2, coarse box i on rank i): every register crosses ranks.  "wrap": the geometry of the other tests -- the
# wrapped register reaches a flux FAB of either rank.
_RANK_PATCHES = {"seam": [((4, 2, 2), (7, 5, 5)), ((8, 2, 2), (11, 5, 5))], "wrap": R.FINE}


def _ranks_run(comm, which):
    from oracle import oracle_lib as O
    a = R.make_amr(R.RefluxOracleBackend, O.default_params(init_shrink=0.5), True, patches=[_RANK_PATCHES[which]], comm=comm,
                   do_grav=True, const_grav=-2.0, rotation=_rotation())
    R.init_state(a)
    dts = [a.step() for _ in range(2)]
    return a, dts


def _ranks_worker(rank, world, port, which, out_path):
    import torch.distributed as dist
    import castro_amd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        a, dts = _ranks_run(castro_amd.DistComm(), which)
        if which == "seam":
            for f in a.lev[1].boxes:
                under = [p for p in a.lev[0].boxes if p.lo[0] <= f.pbox[0][0] <= p.hi[0]]
                assert len(under) == 1 and under[0].owner != f.owner
        levels = [a.gather_level(l) for l in range(len(a.lev))]
        if rank == 0:
            pickle.dump(dict(dts=dts, data=levels), open(out_path, "wb"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("which", list(_RANK_PATCHES))
def test_two_ranks_equal_one_bit_for_bit_gloo(tmp_path, oracle, which):
    """gloo, world 2, option on, gravity and rotation, two coarse steps: the registers travel to the owners of the coarse flux
    FABs (the _xrun kind reg_to_flux); dt sequence and every box of every level equal the one-rank run bit for bit."""
    out = str(tmp_path / "reflux_sources_ranks.pkl")
    mp.spawn(_ranks_worker, args=(2, _free_port(), which, out), nprocs=2, join=True)
    got = pickle.load(open(out, "rb"))
    a, dts = _ranks_run(None, which)
    assert got["dts"] == dts
    for l, lev in enumerate(a.lev):
        assert [bx for bx, _ in got["data"][l]] == [b.bx for b in lev.boxes]
        for (bx, arr), b in zip(got["data"][l], lev.boxes):
            assert np.array_equal(arr, b.S_new().numpy()), "level %d box %s" % (l, bx)


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def test_the_default_is_off_and_the_single_level_driver_has_no_such_keyword(oracle):
    import castro_amd
    a = R.make_amr(R.RefluxOracleBackend, _params(oracle), False)
    b = castro_amd.CastroAmr(R.N_CELL, patches=[R.FINE], prob_hi=R.PROB_HI, params=_params(oracle), make_hydro=R.RefluxOracleBackend,
                             base_grid=R.BASE_GRID, **R.PERIODIC_X)
    assert a.update_sources_after_reflux is False and b.update_sources_after_reflux is False
    with pytest.raises(TypeError):
        castro_amd.Castro((16, 16, 16), params=_params(oracle), hydro=R.RefluxOracleBackend(), update_sources_after_reflux=True)


def test_the_library_exports_the_new_entry_point_and_operation():
    from castro_amd import _lib
    assert "castro_amd_fluxreg_to_flux_fab" in _lib.EXPORTED_SYMBOLS and _lib.OP_FLUXREG_TO_FLUX == 9
    assert _lib.SOURCES_AFTER_REFLUX == 16
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "castro_hydro_amd.h")).read()
    assert "#define CASTRO_AMD_SOURCES_AFTER_REFLUX 16" in hdr and "#define CASTRO_AMD_OP_FLUXREG_TO_FLUX 9" in hdr and "int castro_amd_fluxreg_to_flux_fab(" in hdr

"""Checkpoint and restart (castro_amd/checkpoint.py) on the CPU backend, with the torch fallback of the pack: the on-disk format,
and the yardstick -- a run checkpointed at step k, thrown away, restarted from the directory and continued to step n leaves the
bits of the run that went to n without stopping.  Every comparison is bitwise."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.oracle_backend import OracleBackend
from tests.test_driver_cpu import _free_port

N16 = (16, 16, 16)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def _same(a, b, what):
    a, b = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (a, b))
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b), what


def compare_single(a, b, bookkeeping=True):
    """two Castro objects: the valid zones of S_new, time, dt, nstep and where present new_source, the point mass, the particles;
    bookkeeping: lastDt and nsubcycles too (not between a run that went through step() and one that never did: run_steps does
    not count subcycles)"""
    _same(a.S_new(), b.S_new(), "S_new")
    assert (a.time, a.dt, a.nstep) == (b.time, b.dt, b.nstep)
    if bookkeeping:
        assert (a.lastDt, a.nsubcycles) == (b.lastDt, b.nsubcycles)
    if a.have_sources:
        _same(a.new_source, b.new_source, "new_source")
    if a.pm is not None:
        assert a.point_mass == b.point_mass
    if a.tracers is not None:
        for k in ("pos", "r", "ints", "flags"):
            _same(getattr(a.tracers, k), getattr(b.tracers, k), "tracers." + k)


def compare_amr(a, b):
    assert [lev.box_list() for lev in a.lev] == [lev.box_list() for lev in b.lev]
    assert (a.time, a.nstep, a.dt_level, a.level_count) == (b.time, b.nstep, b.dt_level, b.level_count)
    for la, lb in zip(a.lev, b.lev):
        assert la.lastDt == lb.lastDt
        for x, y in zip(la.boxes, lb.boxes):
            _same(x.S_new(), y.S_new(), "S_new of box %s of level %d" % (x.bx, la.l))
            if x.have_sources:
                _same(x.new_source, y.new_source, "new_source of box %s of level %d" % (x.bx, la.l))
    if a.pm is not None:
        assert a.point_mass == b.point_mass
    if a.tracers is not None:
        for k in ("pos", "r", "ints", "flags"):
            _same(getattr(a.tracers, k), getattr(b.tracers, k), "tracers." + k)


def continuation(make, init, tmp_path, nsteps=6, at=3, compare=compare_single, step=lambda c: c.step()):
    """run a: init, nsteps steps.  run b: `at` steps, writeCheckpoint, the object deleted, a new one, restart, the rest."""
    a = make()
    init(a)
    for _ in range(nsteps):
        step(a)
    b = make()
    init(b)
    for _ in range(at):
        step(b)
    d = str(tmp_path / ("chk%05d" % at))
    assert b.writeCheckpoint(d) == d
    assert not os.path.exists(d + ".temp")
    nstep = b.nstep
    del b
    c = make()
    c.restart(d)
    assert c.nstep == nstep and c.diag_history == []
    for _ in range(nsteps - at):
        step(c)
    compare(a, c)
    return a, c, d


def _sedov(oracle, **kw):
    import castro_amd
    return lambda: castro_amd.Castro(N16, params=oracle.default_params(), hydro=OracleBackend(), **kw)


def _sedov_init(c):
    c.initData("sedov", r_init=0.1, nsub=4)


# ---- 1. format ----------------------------------------------------------------------------------------------------------------
def test_format(oracle, tmp_path):
    from castro_amd import checkpoint as CK
    from castro_amd import plotfile as PF
    c = _sedov(oracle)()
    _sedov_init(c)
    for _ in range(3):
        c.step()
    c.check_file = str(tmp_path / "chk")
    d = c.writeCheckpoint()
    assert d == str(tmp_path / "chk00003") and sorted(os.listdir(str(tmp_path))) == ["chk00003"]      # no .temp left
    rd = lambda name: open(os.path.join(d, name), "rb").read()
    assert rd("CastroHeader") == b"Checkpoint version: 10\n"
    assert rd("state_names.txt") == b"density\nxmom\nymom\nzmom\nrho_E\nrho_e\nTemp\nrho_X\n"
    assert not os.path.exists(os.path.join(d, "point_mass")) and not os.path.exists(os.path.join(d, "Particles"))
    cpu = rd("CPUtime").decode()
    assert cpu == "%.17g" % float(cpu) and float(cpu) >= 0.0                # 17 significant digits, no newline
    assert rd("job_info").decode() == PF.job_info_text(1, N16, 3, c.time, c.geom, c.params)
    assert sorted(os.listdir(os.path.join(d, "Level_0"))) == ["SD_0_New_MF_D_00000", "SD_0_New_MF_H"]
    H = rd("Header").decode().split("\n")
    assert H[:5] == ["CheckPointVersion_1.0", "3", "%.17g" % c.time, "0", "0"] and float(H[2]) == c.time
    ck = CK.read_checkpoint(d)
    assert ck["version"] == 10 and ck["state_names"] == PF.STATE_NAMES and ck["max_level"] == 0 and ck["finest_level"] == 0
    assert (ck["time"], ck["dt"], ck["nstep"]) == (c.time, c.dt, 3)         # == on Python floats: the same bits
    assert ck["dt_level"] == [c.dt] and ck["level_steps"] == [3]
    lev = ck["levels"][0]
    assert lev["boxes"] == [((0, 0, 0), (15, 15, 15))] and lev["source"] is None
    S = c.S_new().numpy()
    assert np.array_equal(_bits(lev["state"][0]), _bits(S))
    # every FabOnDisk offset and min / max of the VisMF header agrees with the data
    (b,) = lev["headers"][0]
    assert (b["file"], b["offset"]) == ("SD_0_New_MF_D_00000", 0)
    raw = rd("Level_0/SD_0_New_MF_D_00000")
    head = ("FAB %s((0,0,0) (15,15,15) (0,0,0)) 8\n" % PF.FAB_REAL_DESCRIPTOR).encode()
    assert raw[:len(head)] == head and raw[len(head):] == np.ascontiguousarray(S, dtype="<f8").tobytes()
    assert b["min"] == [float("%.16e" % S[n].min()) for n in range(8)] and b["max"] == [float("%.16e" % S[n].max()) for n in range(8)]
    assert b["min"] == [float(S[n].min()) for n in range(8)]                # 17 significant digits read back to the same double
    drv = json.load(open(os.path.join(d, "castro_amd_state.json")))
    assert float.fromhex(drv["dt"]) == c.dt and float.fromhex(drv["lastDt"]) == c.lastDt
    assert (None if drv["next_est"] is None else float.fromhex(drv["next_est"])) == c._next_est


# ---- 2. continuation, single level --------------------------------------------------------------------------------------------
def test_continuation_sedov(oracle, tmp_path):
    continuation(_sedov(oracle), _sedov_init, tmp_path)


def test_continuation_constant_gravity_with_predictor(oracle, tmp_path):
    import castro_amd
    make = lambda: castro_amd.Castro(N16, params=oracle.default_params(source_term_predictor=1), hydro=OracleBackend(), do_grav=True,
                                     const_grav=-1.0)
    a, c, d = continuation(make, _sedov_init, tmp_path)
    assert a.have_sources and float(a.new_source.abs().max()) > 0.0
    from castro_amd.checkpoint import read_checkpoint
    ck = read_checkpoint(d)
    assert sorted(os.listdir(os.path.join(d, "Level_0"))) == ["SD_0_New_MF_D_00000", "SD_0_New_MF_H", "SD_3_New_MF_D_00000", "SD_3_New_MF_H"]
    assert ck["levels"][0]["source"][0].shape == (7, 16, 16, 16)


def test_continuation_monopole_point_mass(oracle, tmp_path):
    import castro_amd
    from tests import monopole_ref as R
    from tests import pointmass_ref as PR

    def make():
        c = castro_amd.Castro(R.DUST_N, params=oracle.default_params(**R.DUST_PARAMS), hydro=PR.PointMassOracleBackend(), do_grav=True,
                              gravity_type="monopole", drdxfac=R.DUST_DRDXFAC, use_point_mass=True, point_mass=1.e30,
                              point_mass_fix_solution=True, **R.DUST_GEOM)
        c.center = (0.0, 0.0, 0.0)
        return c
    a, c, d = continuation(make, lambda c: c.initData("dust_collapse", **R.DUST_PROB), tmp_path)
    assert a.point_mass != 1.e30, "the case must move mass into the point mass"
    assert open(os.path.join(d, "point_mass")).read().endswith("\n")
    from castro_amd.checkpoint import read_checkpoint
    pm = read_checkpoint(d)["point_mass"]
    assert open(os.path.join(d, "point_mass")).read() == "%.17g\n" % pm


def test_continuation_rotation_and_sponge(oracle, tmp_path):
    import castro_amd
    from castro_amd import _lib
    from tests import sponge_ref as S
    rot = _lib.make_rotation(rotational_period=2.0, rot_axis=3)
    sp = _lib.make_sponge(1.e-2, lower_radius=0.05, upper_radius=0.3)
    make = lambda: castro_amd.Castro(N16, params=oracle.default_params(init_shrink=0.1), hydro=S.SpongeOracleBackend(), rotation=rot, sponge=sp)
    a, _, _ = continuation(make, _sedov_init, tmp_path)
    assert a.have_sources


def _tracer_positions(n=50, seed=77):
    return np.random.default_rng(seed).uniform(0.2, 0.8, size=(n, 3))


def test_continuation_tracers(oracle, tmp_path):
    import castro_amd
    from tests.tracer_backend import TracerOracleBackend
    ts = {"n": 0}

    def make():
        ts["n"] += 1
        tr = castro_amd.TracerParticles(positions=_tracer_positions(), timestamp_dir=str(tmp_path / ("ts%d" % min(ts["n"], 2))))
        return castro_amd.Castro(N16, hydro=TracerOracleBackend(), params=oracle.default_params(init_shrink=0.1), tracers=tr)
    a, c, d = continuation(make, _sedov_init, tmp_path)
    assert not np.array_equal(a.tracers.positions(), _tracer_positions())
    assert sorted(os.listdir(os.path.join(d, "Particles"))) == ["DATA_00000", "Header"]
    # the restarted run appends to the timestamp file of the run it continues (runs b and c share ts2)
    assert open(str(tmp_path / "ts1" / "Timestamp_00")).read() == open(str(tmp_path / "ts2" / "Timestamp_00")).read()


# ---- 3. continuation with a retry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [3, 4])
def test_continuation_with_a_retry(oracle, tmp_path, at):
    """the retry case of test_source_term_predictor_matches_the_oracle_driver_and_changes_the_answer (tests/test_driver_cpu.py,
    init_shrink = 1): a perturbed hydrostatic column under gravity with the source-term predictor, whose step 4 fails its
    validity check and is redone as two subcycles -- lastDt is then the subcycle's, and the attempt after the rejection makes
    no new corrector"""
    import castro_amd
    from tests.test_driver_cpu import _hse_atmosphere
    n = (4, 4, 32)
    S0 = _hse_atmosphere(n)
    S0[3] = S0[0] * 0.2 * np.random.default_rng(5).uniform(-1, 1, size=S0[0].shape)
    S0[4] += 0.5 * S0[3] ** 2 / S0[0]
    pkw = dict(source_term_predictor=1, init_shrink=1.0, change_max=1.05)
    make = lambda: castro_amd.Castro(n, params=oracle.default_params(**pkw), hydro=OracleBackend(), do_grav=True, const_grav=-20.0,
                                     lo_bc=(4, 4, 3), hi_bc=(4, 4, 3), prob_hi=(0.125, 0.125, 1.0))
    seen = []

    def step(c):
        c.step(1.0)
        seen.append((c.nstep, c.nsubcycles, c.nretries))
    a, c, _ = continuation(make, lambda c: c.set_state(S0.copy()), tmp_path, nsteps=6, at=at, step=step)
    assert (4, 2, 1) in seen[:6], "step 4 must subcycle: %r" % (seen,)
    assert a.lastDt != a.dt                                                 # the last step subcycled too: lastDt is the subcycle's


# ---- 4. continuation, AMR -----------------------------------------------------------------------------------------------------
def _amr_run(make, init, tmp_path, nsteps=4, at=2):
    a, c, d = continuation(make, init, tmp_path, nsteps=nsteps, at=at, compare=compare_amr)
    return a, c, d


_SOD = dict(rho_l=1.0, u_l=0.0, p_l=1.0, rho_r=0.125, u_r=0.0, p_r=0.1)


@pytest.mark.parametrize("problem", ["sod", "sedov"])
def test_continuation_amr(oracle, tmp_path, problem):
    """checkpoint at 2 of 4 coarse steps with regrid_int = 2: a regrid is due at the start of step 3, so level_count matters.
    sod: the density jump is refined from the start, the checkpoint holds two levels.  sedov (uniform density at first): the
    checkpoint holds level 0 alone and the regrid of step 3 -- which a run that lost level_count would not make -- adds level 1."""
    import castro_amd
    from castro_amd.checkpoint import read_checkpoint
    make = lambda: castro_amd.CastroAmr(N16, max_level=1, refine=[("density", "gradient", 0.01)], regrid_int=2,
                                        params=oracle.default_params(init_shrink=1.0), make_hydro=OracleBackend)
    init = (lambda x: x.initData("sod", **_SOD)) if problem == "sod" else _sedov_init
    a, c, d = _amr_run(make, init, tmp_path)
    assert len(a.lev) == 2
    ck = read_checkpoint(d)
    finest = 1 if problem == "sod" else 0
    assert ck["max_level"] == 1 and ck["finest_level"] == finest and len(ck["levels"]) == finest + 1
    assert ck["level_count"] == [2, 4 * finest]                             # a regrid is due at the restart
    assert ck["dt_level"][1] == ck["dt_level"][0] / 2 and ck["level_steps"] == [2, 4]
    # the box lists after the restart equal those before it
    b = make()
    b.restart(d)
    assert [lev.box_list() for lev in b.lev] == [lv["boxes"] for lv in ck["levels"]]
    assert b.level_count[:2] == [2, 4 * finest] and b.nstep == 2 and b.dt_level == [float(x) for x in b.dt_level]
    if problem == "sod":
        assert b.lev[1].box_list() == [((8, 0, 0), (23, 31, 31))]
        for x, y in zip(b.lev[1].boxes, ck["levels"][1]["state"]):
            assert np.array_equal(_bits(x.S_new().numpy()), _bits(y))


def test_continuation_amr_monopole_after_reflux_sources(oracle, tmp_path):
    import castro_amd
    from tests import monopole_amr_ref as A
    from tests import monopole_ref as R
    from tests import reflux_sources_ref as RS

    class Backend(RS.RegToFlux, A.MonopoleAmrOracleBackend):
        pass

    def make():
        g = castro_amd.MonopoleGravity(drdxfac=A.AMR_DRDXFAC, center=(0.0, 0.0, 0.0))
        return castro_amd.CastroAmr(N16, max_level=1, refine=[("density", "gradient", 0.01)], regrid_int=2,
                                    params=oracle.default_params(**R.DUST_PARAMS), make_hydro=Backend, do_grav=True, gravity=g,
                                    update_sources_after_reflux=True, **R.DUST_GEOM)
    a, c, d = _amr_run(make, lambda x: x.initData("dust_collapse", **R.DUST_PROB), tmp_path)
    assert len(a.lev) == 2 and a.lev[0].have_sources
    assert "SD_3_New_MF_H" in os.listdir(os.path.join(d, "Level_1"))


# ---- 5. two gloo ranks ---------------------------------------------------------------------------------------------------------
def _two_rank_case(comm, tmp, ckpt):
    """Castro 16^3 on a 2 x 1 x 1 grid, periodic in x with a bulk x velocity: tracers cross the rank boundary"""
    import castro_amd
    from oracle import oracle_lib as O
    from tests import tracer_migrate_cases as K
    from tests.tracer_migrate_backend import TracerMigrateOracleBackend

    def make(tag):
        tr = castro_amd.TracerParticles(positions=K.single_positions(2), timestamp_dir=os.path.join(tmp, "ts_" + tag))
        return castro_amd.Castro(N16, grid=(2, 1, 1), lo_bc=(0, 2, 2), hi_bc=(0, 2, 2), comm=comm, tracers=tr,
                                 hydro=TracerMigrateOracleBackend(), params=O.default_params(init_shrink=1.0))
    init = lambda c: c.initData("sod", rho_l=1.0, u_l=1.0, p_l=1.0, rho_r=0.125, u_r=1.0, p_r=0.1)
    a = make("a")
    init(a)
    ids0 = sorted(int(x) for x in a.tracers.ints[0].tolist())
    for _ in range(4):
        a.step()
    b = make("b")
    init(b)
    b.step(), b.step()
    b.writeCheckpoint(ckpt)
    del b
    c = make("b")
    c.restart(ckpt)
    c.step(), c.step()
    compare_single(a, c)
    return ids0, sorted(int(x) for x in c.tracers.ints[0].tolist())


def _two_rank_worker(rank, world, port, tmp):
    import torch.distributed as dist
    import castro_amd
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ids0, ids1 = _two_rank_case(castro_amd.DistComm(), tmp, os.path.join(tmp, "chk00002"))
        with open(os.path.join(tmp, "ok_%d" % rank), "w") as f:
            json.dump([ids0, ids1], f)
    finally:
        dist.destroy_process_group()


def test_continuation_two_gloo_ranks(oracle, tmp_path):
    tmp = str(tmp_path)
    mp.spawn(_two_rank_worker, args=(2, _free_port(), tmp), nprocs=2, join=True)
    ids = [json.load(open(os.path.join(tmp, "ok_%d" % r))) for r in range(2)]        # per rank: ids after initData, ids at the end
    assert sorted(ids[0][0] + ids[1][0]) == list(range(1, 201)) == sorted(ids[0][1] + ids[1][1])
    moved = set(ids[0][0]) & set(ids[1][1]) | set(ids[1][0]) & set(ids[0][1])
    assert len(moved) >= 5, "tracers must cross the rank boundary: %d did" % len(moved)
    d = os.path.join(tmp, "chk00002")
    assert not os.path.exists(d + ".temp")
    assert sorted(os.listdir(os.path.join(d, "Level_0"))) == ["SD_0_New_MF_D_00000", "SD_0_New_MF_D_00001", "SD_0_New_MF_H"]
    assert sorted(os.listdir(os.path.join(d, "Particles"))) == ["DATA_00000", "DATA_00001", "Header"]
    from castro_amd.checkpoint import read_checkpoint
    ck = read_checkpoint(d)
    assert ck["levels"][0]["boxes"] == [((0, 0, 0), (7, 15, 15)), ((8, 0, 0), (15, 15, 15))]
    assert [b["file"] for b in ck["levels"][0]["headers"][0]] == ["SD_0_New_MF_D_00000", "SD_0_New_MF_D_00001"]
    assert sum(ck["particles"]["counts"]) == 200


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good(oracle, tmp_path_factory):
    """a good checkpoint of plain Sedov 16^3 after 2 steps, written once and left unchanged"""
    d = str(tmp_path_factory.mktemp("good") / "chk00002")
    c = _sedov(oracle)()
    _sedov_init(c)
    c.step(), c.step()
    c.writeCheckpoint(d)
    return d


def _copy(good, tmp_path):
    d = str(tmp_path / "chk")
    shutil.copytree(good, d)
    return d


def _edit(d, name, fn):
    p = os.path.join(d, name)
    s = open(p).read()
    t = fn(s)
    assert t != s
    open(p, "w").write(t)


def test_restart_refusals(oracle, good, tmp_path):
    import castro_amd
    from castro_amd import _lib
    from tests.tracer_backend import TracerOracleBackend
    P = oracle.default_params
    mk = lambda n=N16, **kw: castro_amd.Castro(n, params=P(), hydro=OracleBackend(), **kw)
    mk().restart(good)                                                      # the good one is good
    with pytest.raises(ValueError, match="n_cell"):
        mk((16, 16, 8)).restart(good)
    with pytest.raises(ValueError, match="prob_lo"):
        mk(prob_lo=(-1., 0., 0.)).restart(good)
    with pytest.raises(ValueError, match="prob_hi"):
        mk(prob_hi=(2., 1., 1.)).restart(good)
    with pytest.raises(ValueError, match="periodicity"):
        mk(lo_bc=(0, 2, 2), hi_bc=(0, 2, 2)).restart(good)
    with pytest.raises(ValueError, match="source terms"):
        mk(do_grav=True, const_grav=-1.0).restart(good)
    with pytest.raises(ValueError, match="tracer particles on one side"):
        castro_amd.Castro(N16, params=P(), hydro=TracerOracleBackend(), tracers=castro_amd.TracerParticles(positions=_tracer_positions())).restart(good)
    with pytest.raises(ValueError, match="CastroAmr|written by a Castro"):
        castro_amd.CastroAmr(N16, patch_crse=((4, 4, 4), (11, 11, 11)), params=P(), make_hydro=OracleBackend).restart(good)
    d = _copy(good, tmp_path / "v")
    _edit(d, "CastroHeader", lambda s: s.replace("10", "9"))
    with pytest.raises(ValueError, match="version 9"):
        mk().restart(d)
    d = _copy(good, tmp_path / "n")
    _edit(d, "state_names.txt", lambda s: s.replace("rho_X", "rho_He4"))
    with pytest.raises(ValueError, match="state names"):
        mk().restart(d)
    d = _copy(good, tmp_path / "r")
    _edit(d, "castro_amd_state.json", lambda s: s.replace('"nranks": 1', '"nranks": 2'))
    with pytest.raises(ValueError, match="number of ranks"):
        mk().restart(d)
    d = _copy(good, tmp_path / "g")
    _edit(d, "castro_amd_state.json", lambda s: json.dumps(dict(json.loads(s), grid=[1, 1, 2])))
    with pytest.raises(ValueError, match="rank grid"):
        mk().restart(d)
    # the reverse of the source-term case: a checkpoint with Source_Type data, a run without
    g = mk(do_grav=True, const_grav=-1.0)
    _sedov_init(g)
    g.step()
    d = g.writeCheckpoint(str(tmp_path / "src"))
    with pytest.raises(ValueError, match="no source terms"):
        mk().restart(d)
    with pytest.raises(ValueError, match="tracer particles on one side"):
        t = castro_amd.Castro(N16, params=P(), hydro=TracerOracleBackend(), tracers=castro_amd.TracerParticles(positions=_tracer_positions()))
        _sedov_init(t)
        t.step()
        mk().restart(t.writeCheckpoint(str(tmp_path / "tr")))


def test_continuation_amr_static_patch_with_tracers(oracle, tmp_path):
    """CastroAmr with a fixed refined box (patches: the levels are not rebuilt from the file, their boxes are compared with it)
    and tracers across both levels: TracerParticles.restore on a hierarchy; another patch is refused by name"""
    import castro_amd
    from tests.tracer_backend import TracerOracleBackend
    patch = ((4, 4, 4), (11, 11, 11))
    pos = np.random.default_rng(78).uniform(0.1, 0.9, size=(40, 3))
    mk = lambda pc=patch: castro_amd.CastroAmr(N16, pc, params=oracle.default_params(init_shrink=0.1), make_hydro=TracerOracleBackend,
                                               tracers=castro_amd.TracerParticles(positions=pos))
    a, c, d = continuation(mk, _sedov_init, tmp_path, nsteps=4, at=2, compare=compare_amr)
    lv = a.tracers.levels()
    assert set(lv.tolist()) == {0, 1} and not np.array_equal(a.tracers.positions(), pos)
    assert sorted(os.listdir(os.path.join(d, "Particles"))) == ["DATA_00000", "Header"]
    with pytest.raises(ValueError, match="boxes of level 1 differ"):
        mk(((2, 4, 4), (9, 11, 11))).restart(d)


def test_nan_in_a_valid_zone_propagates_into_min_and_max(tmp_path):
    """the one rule of every path that fills a VisMF header: a NaN in a valid zone makes the minimum and the maximum of its
    (FAB, component) NaN -- the torch form of the pack here, numpy's in the plotfile writer; the kernel: tests/test_checkpoint_gpu.py"""
    from castro_amd import checkpoint as CK
    from castro_amd import plotfile as PF
    t = torch.arange(2 * 4 * 4 * 4, dtype=torch.float64).reshape(2, 4, 4, 4) + 1.0
    t[1, 2, 1, 1] = float("nan")
    dst, mm = torch.zeros(2 * 8), torch.zeros(4)
    CK.pack(object(), [(t, ((0, 0, 0), (3, 3, 3)), ((1, 1, 1), (2, 2, 2)))], dst, mm)
    assert mm[0].item() == 22.0 and mm[2].item() == 43.0 and np.isnan(mm[1].item()) and np.isnan(mm[3].item())
    mn, mx = PF.fab_minmax(t[:, 1:3, 1:3, 1:3].numpy())
    assert mn[0] == 22.0 and mx[0] == 43.0 and np.isnan(mn[1]) and np.isnan(mx[1])


def test_restart_refuses_a_finest_level_above_max_level(oracle, tmp_path):
    import castro_amd
    mk = lambda max_level: castro_amd.CastroAmr(N16, max_level=max_level, refine=[("density", "gradient", 0.01)], regrid_int=2,
                                                params=oracle.default_params(), make_hydro=OracleBackend)
    a = mk(1)
    a.initData("sod", **_SOD)
    a.step()
    assert len(a.lev) == 2
    d = a.writeCheckpoint(str(tmp_path / "chk00001"))
    with pytest.raises(ValueError, match="finest_level 1 .* max_level 0"):
        mk(0).restart(d)
    with pytest.raises(ValueError, match="n_cell"):
        castro_amd.CastroAmr((8, 8, 8), max_level=1, refine=[("density", "gradient", 0.01)], params=oracle.default_params(),
                             make_hydro=OracleBackend).restart(d)


# ---- 7. check_int ---------------------------------------------------------------------------------------------------------------
def test_check_int(oracle, tmp_path):
    import castro_amd
    mk = lambda **kw: castro_amd.Castro(N16, params=oracle.default_params(), hydro=OracleBackend(), diag_dir=str(tmp_path / "diag"),
                                        sum_interval=-1, **kw)
    probe = mk()
    _sedov_init(probe)
    probe.evolve(1.0, max_step=5)
    stop = probe.time - 0.25 * probe.dt                                     # inside step 5: evolve clips its last step to it
    a = mk()
    _sedov_init(a)
    a.evolve(stop)
    assert a.nstep == 5 and a.time == stop
    b = mk(check_int=2, check_file=str(tmp_path / "chk"))
    _sedov_init(b)
    b.evolve(stop)
    assert b.nstep == 5
    b.close()                                                               # joins the background write
    assert sorted(x for x in os.listdir(str(tmp_path)) if x.startswith("chk")) == ["chk00002", "chk00004"]
    compare_single(a, b)                                                    # writing checkpoints changes nothing
    c = mk(check_int=2, check_file=str(tmp_path / "again"))
    c.restart(str(tmp_path / "chk00004"))
    c.evolve(stop)
    c.close()
    compare_single(a, c)
    assert not any(x.startswith("again") for x in os.listdir(str(tmp_path)))    # step 5 is no multiple of 2, step 4 was not taken here


def test_restarted_run_appends_to_the_diagnostics(oracle, tmp_path):
    import castro_amd
    from tests.test_diag_cpu import DiagOracleBackend
    mk = lambda d: castro_amd.Castro(N16, params=oracle.default_params(), hydro=DiagOracleBackend(), diag_dir=str(tmp_path / d), sum_interval=1)
    a = mk("a")
    _sedov_init(a)
    for _ in range(4):
        a.step()
    b = mk("b")
    _sedov_init(b)
    b.step(), b.step()
    d = b.writeCheckpoint(str(tmp_path / "chk00002"))
    del b
    c = mk("b")
    c.restart(d)
    assert c.diag_history == []
    c.step(), c.step()
    assert len(c.diag_history) == 2
    for name in ("grid_diag.out", "species_diag.out"):                      # amr_diag.out carries wall times
        assert open(str(tmp_path / "a" / name)).read() == open(str(tmp_path / "b" / name)).read(), name
    assert len(open(str(tmp_path / "b" / "amr_diag.out")).read().split("\n")) == len(open(str(tmp_path / "a" / "amr_diag.out")).read().split("\n"))


# ---- 8. a failing background write ---------------------------------------------------------------------------------------------
def test_failing_background_write(oracle, tmp_path):
    ro = tmp_path / "readonly"
    ro.mkdir()
    os.chmod(str(ro), 0o555)
    target = str(ro / "chk")
    if os.access(str(ro), os.W_OK):
        # a superuser writes through the mode bits: a path under a regular file is as unwritable for everybody
        (tmp_path / "file").write_text("x")
        target = str(tmp_path / "file" / "chk")
    a = _sedov(oracle)()
    _sedov_init(a)
    b = _sedov(oracle)()
    _sedov_init(b)
    b.check_file = target
    for c in (a, b):
        c.step(), c.step()
    try:
        b.writeCheckpoint(background=True)                                  # returns: the error belongs to the thread
        b.step()
        with pytest.raises(OSError):
            b.checkpoint_wait()
        b.checkpoint_wait()                                                 # raised once
        a.step()
        b.step(), a.step()
        compare_single(a, b)                                                # the run's state is unharmed
        b.close()
    finally:
        os.chmod(str(ro), 0o755)


# ---- background writes on more than one rank: the thread only writes, the next collective call finishes -------------------------
def _bg_worker(rank, world, port, tmp):
    import torch.distributed as dist
    import castro_amd
    from oracle import oracle_lib as O
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mk = lambda **kw: castro_amd.Castro(N16, grid=(2, 1, 1), comm=castro_amd.DistComm(), hydro=OracleBackend(),
                                            params=O.default_params(), **kw)
        c = mk(check_int=2, check_file=os.path.join(tmp, "chk"))
        _sedov_init(c)
        c.evolve(1.0, max_step=5)
        c.close()                               # the barrier and the rename of chk00004 happen here
        r = mk()
        r.restart(os.path.join(tmp, "chk00004"))
        r.step()
        compare_single(c, r)
        open(os.path.join(tmp, "ok_%d" % rank), "w").close()
    finally:
        dist.destroy_process_group()


def test_check_int_two_gloo_ranks(oracle, tmp_path):
    tmp = str(tmp_path)
    mp.spawn(_bg_worker, args=(2, _free_port(), tmp), nprocs=2, join=True)
    assert sorted(os.listdir(tmp)) == ["chk00002", "chk00004", "ok_0", "ok_1"]

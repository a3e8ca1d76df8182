"""Tracer particles on more than one rank, on the CPU: the numpy restatement of the migration (tests/tracer_migrate_ref.py)
against known answers, and Castro / CastroAmr runs on 2 and 3 gloo ranks with the CPU backend (tests/tracer_migrate_backend.py)
against the same runs on one rank -- particles, files and time steps bit for bit (tests/tracer_migrate_cases.py)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import tracer_migrate_cases as K
from tests import tracer_migrate_ref as M
from tests import tracer_ref as R
from tests.test_driver_cpu import _free_port

# two levels: three boxes dealt to ranks 0, 1, 2 and two boxes dealt to ranks 2, 0
OWNERS = [[0, 1, 2], [2, 0]]


def _particles(n, seed):
    rng = np.random.default_rng(seed)
    P = R.particles(rng.uniform(size=(n, 3)))
    P["r0"][:], P["r1"][:], P["r2"][:] = rng.normal(size=(3, n))
    P["cpu"][:] = rng.integers(0, 5, size=n)
    P["level"][:] = rng.integers(0, 2, size=n)
    P["grid"][:] = [rng.integers(0, len(OWNERS[l])) for l in P["level"]]
    return P


def test_restatement_known_answers():
    P = _particles(12, 3)
    #            stays (rank 1)   to 0     to 2     stays   invalid  grid outside  level outside  to 0    to 2    stays  to 0  negative grid
    P["level"][:] = [0,            0,       0,       0,      0,       0,            2,             1,      1,      0,     0,    0]
    P["grid"][:] = [1,             0,       2,       1,      0,       3,            0,             1,      0,      1,     0,    -1]
    P["id"][4] = -5
    dest, counts = M.destinations(P, OWNERS, 3, 1)
    assert dest.tolist() == [1, 0, 2, 1, 1, 1, 1, 0, 2, 1, 0, 1] and counts.tolist() == [3, 7, 2]
    kept, wire = M.pack(P, dest, 3, 1)
    assert kept["id"].tolist() == [1, 4, -5, 6, 7, 10, 12]                          # the stayers keep their order
    assert wire.shape == (5, 8)
    back = M.empty(5)
    M.unpack(wire, back, 0)
    assert back["id"].tolist() == [2, 8, 11, 3, 9]                                  # rank 0's first, each group in its order
    for k in P:
        assert np.array_equal(back[k], P[k][[1, 7, 10, 2, 8]]), k                   # every field, bit for bit
    assert wire[0, 6] == 2 | (int(P["cpu"][1]) << 32) and wire[0, 7] == 0 | (0 << 32) and wire[4, 7] == 1 | (0 << 32)
    assert wire[:, 0].view(np.float64).tolist() == P["x"][[1, 7, 10, 2, 8]].tolist()

    # a lost particle (locate finds it in no box: level and grid stay) does not move either
    from castro_amd import _lib
    geom = _lib.make_geom((8, 8, 8), (0., 0., 0.), (1., 1., 1.), (2, 2, 2), (2, 2, 2))
    L = R.particles([[0.9, 0.9, 0.9], [0.1, 0.1, 0.1]], level=0, grid=0)
    flags = np.zeros(2, dtype=np.int32)
    R.locate(L, 0, 0, 0, [[((0, 0, 0), (3, 7, 7))]], [geom], flags)                  # the box covers x < 0.5 only
    assert flags.tolist() == [0, 1]
    assert M.destinations(L, [[0]], 2, 0)[0].tolist() == [0, 0]


def test_restatement_arrivals_are_ordered_by_source_rank():
    parts = [_particles(9, 10 + r) for r in range(3)]
    for r, P in enumerate(parts):
        P["id"][:] = 100 * (r + 1) + np.arange(9)
    new = M.migrate(parts, OWNERS)
    assert sum(P["id"].shape[0] for P in new) == 27
    for me, P in enumerate(new):
        src = P["id"] // 100 - 1
        nk = int((src == me).sum())
        assert (src[:nk] == me).all() and (np.diff(src[nk:]) >= 0).all()              # stayers, then ascending sources
        for s in range(3):
            assert (np.diff(P["id"][src == s]) > 0).all()                             # each group in its order at the source
        assert all(OWNERS[l][g] == me for l, g in zip(P["level"], P["grid"]))
    again = M.migrate(new, OWNERS)                                                    # nothing moves a second time
    for P, Q in zip(new, again):
        assert all(np.array_equal(P[k], Q[k]) for k in P)


@pytest.fixture(scope="module")
def one_rank(oracle, tmp_path_factory):
    """the one-rank runs, made once and left unchanged: (case, world) -> (arrays, directory)"""
    cache = {}

    def get(case, world):
        key = (case, world if case == "single" else 0)
        if key not in cache:
            d = str(tmp_path_factory.mktemp("one_%s" % case))
            cache[key] = (K.run(case, None, world, "oracle", None, d), d)
        return cache[key]
    return get


@pytest.mark.parametrize("case,world", [("single", 2), ("single", 3), ("amr", 2), ("amr", 3)])
def test_ranks_equal_one_rank_gloo(oracle, one_rank, tmp_path, case, world):
    """Castro(grid=(world, 1, 1), periodic in x, a bulk x velocity) and CastroAmr(patches=_MR_PATCHES) with tracers on `world`
    gloo ranks: ids, positions, r, levels and grids of all particles in id order after initData and after every step, the dt
    sequence, the timestamp file and the write_ascii file equal those of one rank bit for bit; at least 10 particles change
    owner (one of them through the periodic wrap), and n_local changes."""
    d = str(tmp_path)
    mp.spawn(K.worker, args=(world, _free_port(), case, "oracle", None, d), nprocs=world, join=True)
    one, one_dir = one_rank(case, world)
    K.check(case, dict(np.load(os.path.join(d, "run.npz"))), one, world, d, one_dir)


def _flags_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    import castro_amd
    from oracle import oracle_lib as O
    from tests.tracer_migrate_backend import TracerMigrateOracleBackend
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tr = castro_amd.TracerParticles(positions=K.single_positions(world))
        c = castro_amd.Castro(K.single_n_cell(world), grid=(world, 1, 1), lo_bc=(0, 2, 2), hi_bc=(0, 2, 2), comm=castro_amd.DistComm(),
                              tracers=tr, hydro=TracerMigrateOracleBackend(), params=O.default_params())
        c.initData("sod", rho_l=1.0, u_l=1.0, p_l=1.0, rho_r=0.125, u_r=1.0, p_r=0.1)
        tr.check_flags()                                        # nothing set: nobody raises
        if rank == 1:
            tr.flags[0] = 3
        msg = ""
        try:
            tr.check_flags()
        except RuntimeError as e:
            msg = str(e)
        tr.check_flags()                                        # and the counts are cleared on every rank
        with open(os.path.join(out_dir, "flags_%d" % rank), "w") as f:
            f.write(msg)
        # particle_count: every rank counts its own particles into its own box (box r of the table is rank r's)
        c.writePlotFile(os.path.join(out_dir, "plt"), derive=["particle_count"])
        cnt = tr.count_level(0, c._rank_boxes(), c.geom, mine=[r == rank for r in range(world)])
        assert [x is None for x in cnt] == [r != rank for r in range(world)]
        assert int(cnt[rank].sum()) == tr.n_local
        np.save(os.path.join(out_dir, "count_%d.npy" % rank), cnt[rank].numpy())
    finally:
        dist.destroy_process_group()


def test_every_rank_raises_when_one_rank_has_a_flag_and_ranks_count_their_own_box(oracle, tmp_path):
    mp.spawn(_flags_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        assert "3 particle passes had to clamp" in (tmp_path / ("flags_%d" % rank)).read_text()
    # the counts of the two ranks side by side are the counts of the particles' zones
    pos = K.single_positions(2)
    want = np.zeros((8, 8, 16))
    for x, y, z in pos:
        want[int(z * 8), int(y * 8), int(x * 16)] += 1
    got = np.concatenate([np.load(str(tmp_path / ("count_%d.npy" % rank))) for rank in range(2)], axis=2)
    assert np.array_equal(got, want) and got.sum() == pos.shape[0]


def _order_particles(rank):
    """the particles rank `rank` holds before the migration: ids 100 (rank + 1) + 0 .. n - 1, boxes of every rank, one invalid
    particle and one whose grid is outside the table (both stay)"""
    P = _particles(9 + rank, 50 + rank)
    P["id"][:] = 100 * (rank + 1) + np.arange(9 + rank)
    P["id"][2] = -P["id"][2]
    P["grid"][5] = 7
    return P


def _order_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    import castro_amd
    from tests.tracer_migrate_backend import TracerMigrateOracleBackend
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        P = _order_particles(rank)
        tr = castro_amd.TracerParticles(positions=np.zeros((1, 3)))
        tr.hydro, tr.comm = TracerMigrateOracleBackend(), castro_amd.DistComm()
        tr.pos = torch.from_numpy(np.stack([P[k] for k in M.REALS[:3]]))
        tr.r = torch.from_numpy(np.stack([P[k] for k in M.REALS[3:]]))
        tr.ints = torch.from_numpy(np.stack([P[k] for k in M.INTS]))
        tr._migrate(OWNERS)
        np.savez(os.path.join(out_dir, "order_%d.npz" % rank), pos=tr.pos.numpy(), r=tr.r.numpy(), ints=tr.ints.numpy())
    finally:
        dist.destroy_process_group()


def test_array_order_on_every_rank_after_a_migration(oracle, tmp_path):
    """TracerParticles._migrate on 3 gloo ranks, every rank sending to and receiving from both others: the RAW arrays of every
    rank (not a gather sorted by id) equal the restatement's -- the stayers in their previous order, then the arrivals by
    ascending source rank, each group in its order at the source; every field bit for bit"""
    world = 3
    mp.spawn(_order_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    want = M.migrate([_order_particles(rank) for rank in range(world)], OWNERS)
    for rank in range(world):
        got = np.load(str(tmp_path / ("order_%d.npz" % rank)))
        src = want[rank]["id"] // 100 - 1
        assert set(src[want[rank]["id"] > 0].tolist()) == {0, 1, 2}, "rank %d does not receive from both others" % rank
        assert got["ints"][0].tolist() == want[rank]["id"].tolist(), "ids in order, rank %d" % rank
        for q, k in enumerate(M.REALS):
            a = (got["pos"] if q < 3 else got["r"])[q % 3]
            assert np.array_equal(a.view(np.int64), want[rank][k].view(np.int64)), (rank, k)
        for q, k in enumerate(M.INTS):
            assert np.array_equal(got["ints"][q], want[rank][k]), (rank, k)

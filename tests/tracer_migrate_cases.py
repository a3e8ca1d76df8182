"""The two driver scenarios of the migration tests, shared by tests/test_tracer_migrate_cpu.py (CPU backend over gloo) and
tests/test_tracer_migrate_gpu.py (processes sharing the test GPU over gloo): a single-level periodic run with a bulk velocity
whose particles cross the rank face and wrap through the periodic boundary, and a three-level Sedov run with particles
clustered inside the faces of a level-2 box the blast pushes them through.  A run returns the history of all particles in id
order after initData and after every step; the workers write it where the test reads it.  Tests only."""
import json
import os

import numpy as np

SINGLE_STEPS = 5             # at init_shrink = 1 a step moves a particle about a quarter of a zone
AMR_STEPS = 2
R_INIT = 0.125              # the edge of the hot sphere on the faces y = 0.625 and z = 0.625 of box 2 of level 2


def single_n_cell(world):
    return (8 * world, 8, 8)


def single_positions(world):
    """about 200 particles: behind every rank face and behind the periodic face in x (some within 1e-3 dx of them), the rest
    anywhere"""
    rng = np.random.default_rng(4100 + world)
    dx = 1.0 / (8 * world)
    pos = []
    faces = [(r + 1.0) / world for r in range(world)]           # the last one is the periodic face
    for f in faces:
        for _ in range(8):
            pos.append([f - rng.uniform(0.0, 1.0e-3) * dx, rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.95)])
        for _ in range(40 // world + 8):
            pos.append([f - rng.uniform(0.0, 0.06), rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.95)])
    for _ in range(15):                                         # more behind the first face: the ranks' counts do not balance
        pos.append([faces[0] - rng.uniform(0.0, 0.03), rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.95)])
    while len(pos) < 200:
        pos.append([rng.uniform(0.0, 1.0), rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.95)])
    return np.array(pos)


def amr_positions():
    """about 200 particles: just inside the faces y = 0.625 and z = 0.625 of box 2 of level 2 (level-1 zones (8, 16, 8) ..
    (23, 19, 19)), where the edge of the hot sphere drives them outwards into level 1; around the faces x = 0.5 and y = 0.5
    between the boxes of levels 1 and 2; the rest anywhere in the refined region"""
    rng = np.random.default_rng(4200)
    pos = []
    for _ in range(60):
        pos.append([rng.uniform(0.40, 0.60), 0.625 - rng.uniform(1.0e-6, 1.5e-3), rng.uniform(0.45, 0.55)])
    for _ in range(60):
        pos.append([rng.uniform(0.40, 0.60), rng.uniform(0.51, 0.58), 0.625 - rng.uniform(1.0e-6, 1.5e-3)])
    for _ in range(40):
        p = [rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7)]
        p[int(rng.integers(0, 2))] = 0.5 + rng.uniform(-1.0e-3, 1.0e-3)
        pos.append(p)
    while len(pos) < 200:
        pos.append([rng.uniform(0.15, 0.85), rng.uniform(0.15, 0.85), rng.uniform(0.15, 0.85)])
    return np.array(pos)


def _snapshot(tr):
    pos, r, ints = tr._host()
    return pos.copy(), r.copy(), ints.copy()


def _kw(backend, numerics):
    """(constructor keywords of Castro, of CastroAmr) for the CPU backend ("oracle") or the device (None)"""
    if backend == "oracle":
        from oracle import oracle_lib as O
        from tests.tracer_migrate_backend import TracerMigrateOracleBackend
        return (dict(hydro=TracerMigrateOracleBackend(), params=O.default_params(init_shrink=1.0)),
                dict(make_hydro=TracerMigrateOracleBackend, params=O.default_params(init_shrink=0.1)))
    import castro_amd
    return (dict(numerics=numerics, params=castro_amd.default_params(init_shrink=1.0)),
            dict(make_hydro=lambda: castro_amd.HipHydro(0, numerics=numerics), params=castro_amd.default_params(init_shrink=0.1)))


def run(case, comm, world, backend, numerics, out_dir):
    """the run of `case` ("single" | "amr") on the ranks of comm (None: one rank), laid out for `world` ranks; a dict of arrays:
    dts, and per snapshot pos (S, 3, N), r (S, 3, N), ints (S, 4, N), nloc (S, ranks); owners (json) of the boxes"""
    import castro_amd
    kc, ka = _kw(backend, numerics)
    ts = os.path.join(out_dir, "ts")
    if case == "single":
        tr = castro_amd.TracerParticles(positions=single_positions(world), timestamp_dir=ts)
        c = castro_amd.Castro(single_n_cell(world), grid=(world, 1, 1) if comm is not None else None, lo_bc=(0, 2, 2), hi_bc=(0, 2, 2),
                              comm=comm, tracers=tr, **kc)
        c.initData("sod", rho_l=1.0, u_l=1.0, p_l=1.0, rho_r=0.125, u_r=1.0, p_r=0.1)
        nsteps, owners = SINGLE_STEPS, [list(range(world))]
    else:
        from tests.test_amr_cpu import _MR_PATCHES
        tr = castro_amd.TracerParticles(positions=amr_positions(), timestamp_dir=ts, timestamp_temperature=True)
        c = castro_amd.CastroAmr((16, 16, 16), patches=_MR_PATCHES, comm=comm, tracers=tr, **ka)
        c.initData("sedov", r_init=R_INIT, nsub=4)
        nsteps, owners = AMR_STEPS, [[(i + l) % world if l else 0 for i in range(len(lev.boxes))] for l, lev in enumerate(c.lev)]
        if comm is not None:
            assert owners == [[b.owner for b in lev.boxes] for lev in c.lev]
    gather = (lambda x: [x]) if comm is None else comm.gather_objects
    snaps, nloc, dts = [_snapshot(tr)], [gather(tr.n_local)], []
    for _ in range(nsteps):
        dts.append(c.step())
        snaps.append(_snapshot(tr))
        nloc.append(gather(tr.n_local))
    tr.write_ascii(os.path.join(out_dir, "particles.out"))
    return dict(dts=np.array(dts), pos=np.stack([s[0] for s in snaps]), r=np.stack([s[1] for s in snaps]),
                ints=np.stack([s[2] for s in snaps]), nloc=np.array(nloc), owners=np.array(json.dumps(owners)))


def worker(rank, world, port, case, backend, numerics, out_dir):
    import torch
    import torch.distributed as dist
    import castro_amd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if backend == "oracle":
        torch.set_num_threads(1)
    else:
        torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        got = run(case, castro_amd.DistComm(), world, backend, numerics, out_dir)
        if backend != "oracle":
            torch.cuda.synchronize()
        if rank == 0:
            np.savez(os.path.join(out_dir, "run.npz"), **got)
    finally:
        dist.destroy_process_group()


def owner_history(case, one, world):
    """(S, N) owner rank of every particle at every snapshot of the one-rank run `one`, as the run on `world` ranks deals the
    boxes: the single-level run has one box on one rank, so the box of a particle is the one its position lies in (box r: the
    r-th slab in x); the AMR run has the same boxes on any number of ranks: (level, grid) through the owner table"""
    ints = one["ints"]
    if case == "single":
        nx = single_n_cell(world)[0]
        return np.floor(one["pos"][:, 0, :] * nx).astype(np.int64) // (nx // world)
    owners = json.loads(str(one["owners"]))
    out = np.zeros(ints.shape[::2], dtype=np.int64)
    for s in range(ints.shape[0]):
        out[s] = [owners[l][g] for l, g in zip(ints[s, 2], ints[s, 3])]
    return out


def check(case, got, one, world, got_dir, one_dir):
    """the run on `world` ranks against the one-rank run, bit for bit, files included; and that the case is no vacuous one"""
    for s in range(one["ints"].shape[0]):                       # the figures first, then the assertions
        dp, dr = got["pos"][s] - one["pos"][s], got["r"][s] - one["r"][s]
        print("%s, %d ranks, snapshot %d: %d position and %d r entries differ (largest %.3g and %.3g), %d levels, %d grids"
              % (case, world, s, int((dp != 0).sum()), int((dr != 0).sum()), np.abs(dp).max(), np.abs(dr).max(),
                 int((got["ints"][s, 2] != one["ints"][s, 2]).sum()), int((got["ints"][s, 3] != one["ints"][s, 3]).sum())))
    print("dt:", got["dts"].tolist(), one["dts"].tolist())
    assert np.array_equal(got["dts"], one["dts"])
    for s in range(one["ints"].shape[0]):
        assert np.array_equal(got["ints"][s, 0], one["ints"][s, 0]), "ids, snapshot %d" % s
        assert np.array_equal(got["ints"][s, 1], one["ints"][s, 1]), "cpu, snapshot %d" % s
        assert np.array_equal(got["pos"][s].view(np.int64), one["pos"][s].view(np.int64)), "positions, snapshot %d" % s
        assert np.array_equal(got["r"][s].view(np.int64), one["r"][s].view(np.int64)), "r, snapshot %d" % s
        assert np.array_equal(got["ints"][s, 2], one["ints"][s, 2]), "levels, snapshot %d" % s
    own = owner_history(case, one, world)
    if case == "single":
        # one rank has one box (grid 0 everywhere); on `world` ranks grid is the rank whose slab holds the position
        valid = one["ints"][:, 0, :] > 0
        assert np.array_equal(got["ints"][:, 3, :][valid], own[valid].astype(np.int32))
        assert not one["ints"][:, 3, :].any()
    else:
        assert np.array_equal(got["ints"][:, 3, :], one["ints"][:, 3, :])
    for name in ("particles.out", os.path.join("ts", "Timestamp_00")):
        with open(os.path.join(got_dir, name), "rb") as f, open(os.path.join(one_dir, name), "rb") as g:
            a, b = f.read(), g.read()
        assert a == b and len(a) > 1000, name
    moved = own[1:] != own[:-1]
    assert int(moved.any(axis=0).sum()) >= 10, "particles that change owner: %d" % int(moved.any(axis=0).sum())
    if case == "single":
        wrapped = (own[:-1] == world - 1) & (own[1:] == 0) & (one["pos"][1:, 0, :] < one["pos"][:-1, 0, :])
        assert wrapped.any(), "no particle changes owner through the periodic wrap"
    nloc = got["nloc"]
    assert nloc.shape[1] == world and (nloc.sum(axis=1) == one["ints"].shape[2]).all()
    assert (nloc != nloc[0]).any(), "n_local never changed"
    assert (nloc[0] > 0).all(), "the first Redistribute deals rank 0's particles out"

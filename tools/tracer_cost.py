#!/usr/bin/env python
"""What tracer particles cost a step on one MI355X: the wall time of a 128^3 Sedov step() -- host clock around steps that end
in a device synchronise -- with 0, 10^5 and 10^6 particles, against the same step() of a run without the tracers object.  Every
run takes the same path (step(); a run with tracers never takes the host-free batch), the runs are warmed up and then timed in
alternation, --reps windows of --steps steps each; the median per step with the smallest and the largest window.  With 0
particles the cost is the half-time state (one lincomb and its boundary fill) and the flag read; the particles add the two
advection passes and the Redistribute.  No threshold is set anywhere.  The kernel times of the last tracer run are printed from
the context's profiler in a pass of their own (not part of the timed windows).

The migration leg (--legs migration) times what a Redistribute on more than one rank adds on every rank, on one GPU and
without any transport: castro_amd_tracer_migrate_count, _pack and _unpack of 10^5 and 10^6 particles of which about 1 % leave,
over a synthetic owner table of --ranks ranks -- the arrivals are the rank's own leavers, unpacked behind the stayers.  Host
clock around --msteps rounds queued back to back that end in one device synchronise (the one read of the counts a real
Redistribute makes is not in it: the sizes are read once, before the windows).  What real links add is not measured here.

    python tools/tracer_cost.py [--n 128] [--counts 0 100000 1000000] [--steps 100] [--reps 5] [--numerics contract] [--out file.json]
                                [--legs step migration] [--ranks 8] [--msteps 50]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def migration_leg(a, res):
    import numpy as np
    import torch
    import castro_amd
    from castro_amd import _lib
    h = castro_amd.HipHydro(torch.cuda.current_device(), numerics=a.numerics)
    owners, me = [list(range(a.ranks))], 0
    res["migration"] = []
    for count in [c for c in a.counts if c > 0]:
        rng = np.random.default_rng(count)
        pos = torch.from_numpy(rng.uniform(0.02, 0.98, size=(3, count))).cuda()
        r = torch.zeros((3, count), dtype=torch.float64, device="cuda")
        ints = torch.zeros((4, count), dtype=torch.int32, device="cuda")
        ints[0] = torch.arange(1, count + 1, dtype=torch.int32, device="cuda")
        grid = np.where(rng.uniform(size=count) < 0.01, rng.integers(1, a.ranks, size=count), me).astype(np.int32)
        ints[3] = torch.from_numpy(grid).cuda()
        T = _lib.make_tracers(pos, r, ints)
        dest = torch.empty(count, dtype=torch.int32, device="cuda")
        counts = torch.zeros(a.ranks, dtype=torch.int32, device="cuda")
        h.tracer_migrate_count(owners, a.ranks, me, T, dest, counts)
        c = counts.tolist()
        nkeep, nleave = c[me], count - c[me]
        new = [torch.empty((k, count), dtype=d, device="cuda") for k, d in ((3, torch.float64), (3, torch.float64), (4, torch.int32))]
        out = _lib.make_tracers(*new)
        wire = torch.empty((nleave, 8), dtype=torch.int64, device="cuda")

        def round_():
            h.tracer_migrate_count(owners, a.ranks, me, T, dest, counts)
            h.tracer_migrate_pack(a.ranks, me, T, dest, out, wire)
            h.tracer_unpack(wire, out, nkeep)
        for _ in range(5):
            round_()
        windows = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.msteps):
                round_()
            torch.cuda.synchronize()
            windows.append((time.perf_counter() - t0) / a.msteps * 1e3)
        row = dict(particles=count, leaving=nleave, ranks=a.ranks, ms_per_migration_median=float(np.median(windows)),
                   ms_min=min(windows), ms_max=max(windows))
        # the kernels of this count, in a pass of their own: the profiler's events are kept out of the timed windows
        h.profile(True)
        h.profile_reset()
        for _ in range(3):
            round_()
        torch.cuda.synchronize()
        row["kernels"] = {k: v for k, v in h.profile_report().items() if "tracer" in k}
        h.profile(False)
        res["migration"].append(row)
        print("migration of %d particles (%d leave, %d ranks): %.4f ms for count + pack + unpack (windows %.4f .. %.4f)" % (
            count, nleave, a.ranks, row["ms_per_migration_median"], min(windows), max(windows)))
        for k, v in row["kernels"].items():
            print("  %s: %s" % (k, v))
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["step", "migration"], choices=["step", "migration"])
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--msteps", type=int, default=50)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--counts", type=int, nargs="+", default=[0, 100000, 1000000])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tracer_cost.py measures on the GPU; there is nothing to time without one")
    res = dict(device=torch.cuda.get_device_name(0), numerics=a.numerics)
    if "step" in a.legs:
        step_leg(a, res)
    if "migration" in a.legs:
        migration_leg(a, res)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def step_leg(a, res):
    import numpy as np
    import torch
    import castro_amd
    n = (a.n, a.n, a.n)
    runs = []
    for count in [None] + list(a.counts):               # None: no tracers object at all
        kw = {}
        if count is not None:
            kw["tracers"] = castro_amd.TracerParticles(positions=np.random.default_rng(count).uniform(0.02, 0.98, size=(count, 3)))
        c = castro_amd.Castro(n, numerics=a.numerics, **kw)
        c.initData("sedov", r_init=0.05, nsub=4)
        for _ in range(a.warmup):
            c.step()
        runs.append((count, c, []))
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for count, c, windows in runs:                  # alternating: a drift of the machine meets every run alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                c.step()
            torch.cuda.synchronize()
            windows.append((time.perf_counter() - t0) / a.steps * 1e3)
    res.update(n=a.n, steps=a.steps, reps=a.reps, runs=[])
    base = None
    for count, c, windows in runs:
        med = float(np.median(windows))
        base = med if count is None else base
        row = dict(particles=count, ms_per_step_median=med, ms_min=min(windows), ms_max=max(windows), over_no_tracers_ms=med - base)
        if count is not None:
            row["valid_at_end"] = c.tracers.num_valid
        res["runs"].append(row)
        print("%s: %.3f ms per step (windows %.3f .. %.3f), %+.3f ms over the run without tracers" % (
            "no tracers" if count is None else "%d particles" % count, med, min(windows), max(windows), med - base))
    # kernel times of the largest tracer run, profiler on: a pass of its own
    count, c, _ = runs[-1]
    c.hydro.profile(True)
    c.hydro.profile_reset()
    for _ in range(3):
        c.step()
    torch.cuda.synchronize()
    rep = c.hydro.profile_report()
    res["kernels_of_last_run"] = {k: v for k, v in rep.items() if "tracer" in k or "lincomb" in k}
    for k, v in res["kernels_of_last_run"].items():
        print("  %s: %s" % (k, v))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What tracer particles cost a step on one MI355X: the wall time of a 128^3 Sedov step() -- host clock around steps that end
in a device synchronise -- with 0, 10^5 and 10^6 particles, against the same step() of a run without the tracers object.  Every
run takes the same path (step(); a run with tracers never takes the host-free batch), the runs are warmed up and then timed in
alternation, --reps windows of --steps steps each; the median per step with the smallest and the largest window.  With 0
particles the cost is the half-time state (one lincomb and its boundary fill) and the flag read; the particles add the two
advection passes and the Redistribute.  No threshold is set anywhere.  The kernel times of the last tracer run are printed from
the context's profiler in a pass of their own (not part of the timed windows).

    python tools/tracer_cost.py [--n 128] [--counts 0 100000 1000000] [--steps 100] [--reps 5] [--numerics contract] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--counts", type=int, nargs="+", default=[0, 100000, 1000000])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import castro_amd
    if not torch.cuda.is_available():
        sys.exit("tracer_cost.py measures on the GPU; there is nothing to time without one")
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
    res = dict(device=torch.cuda.get_device_name(0), numerics=a.numerics, n=a.n, steps=a.steps, reps=a.reps, runs=[])
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
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

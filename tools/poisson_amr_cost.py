#!/usr/bin/env python
"""What Poisson gravity on the levels of CastroAmr costs on one MI355X (level solves: castro_amd/gravity.py, k_phi_cf_bc of
castro_amd/csrc/poisson_kernels.hip).  No threshold anywhere.

The dust collapse of Exec/gravity_tests/DustCollapse/inputs_3d_poisson_regtest (amr.max_level = 2) with ONE box per level: --base
zones per direction on level 0, level 1 over its middle half, level 2 over the middle half of level 1 -- three levels of --base^3
zones each.  Reported:
  step      ms per coarse step (windows of --steps coarse steps ending in a device synchronise, --reps of them; a coarse step is
            1 + 2 + 4 level advances, 14 solves), and the same hierarchy with max_solve_level = 0 (no fine solve)
  cycles    V-cycles of the last old- and new-time solve of every level
  launches  kernel launches of one coarse step, counted by the profilers of every context of the hierarchy in a step of its own
            (profiling slows the host: that step's time is not reported), those of the multigrid, and the share of k_phi_cf_bc in
            launches and in kernel time

    python tools/poisson_amr_cost.py [--base 64] [--steps 3] [--reps 3] [--numerics contract] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

GEOM = dict(prob_lo=(0., 0., 0.), prob_hi=(1.5e9, 1.5e9, 1.5e9), lo_bc=(2, 2, 2), hi_bc=(2, 2, 2))
CENTER = (7.5e8, 7.5e8, 7.5e8)
PROB = dict(rho_0=1.e9, r_0=6.5e8, p_0=1.e15, rho_ambient=1.0e-5, smooth_delta=4.e6, nsub=2)
PARAMS = dict(eos_gamma=1.66666, small_dens=1.e-6, small_temp=1.e-3, cfl=0.5, init_shrink=0.1, change_max=1.05)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def make_run(n, numerics, max_solve_level=None):
    import castro_amd
    from castro_amd import _lib
    q = n // 4
    p1 = ((q,) * 3, (3 * q - 1,) * 3)                       # level 1: the middle half of level 0, in level-0 zones
    p2 = ((2 * q + q,) * 3, (2 * q + 3 * q - 1,) * 3)       # level 2: the middle half of level 1, in level-1 zones
    a = castro_amd.CastroAmr((n, n, n), params=_lib.default_params(**PARAMS), patches=[p1, p2], do_grav=True,
                             make_hydro=lambda: castro_amd.HipHydro(0, numerics=numerics),
                             gravity=castro_amd.PoissonGravity(center=CENTER, max_solve_level=max_solve_level), **GEOM)
    a.initData("dust_collapse", **PROB)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/poisson_amr_cost.py measures on a GPU; there is none")
    runs = {"level_solves": make_run(a.base, a.numerics), "max_solve_level_0": make_run(a.base, a.numerics, 0)}
    for r in runs.values():
        r.step()
        r.step()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, r in runs.items():                                # alternating: a drift of the machine meets both alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                r.step()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    r = runs["level_solves"]
    cycles = {l: {w: r.poisson_stats(l)[w]["cycles"] for w in ("old", "new")} for l in range(len(r.lev))}
    for h in r.all_hydros():
        h.profile(True)
        h.profile_reset()
    r.step()
    torch.cuda.synchronize()
    rep = {}
    for h in r.all_hydros():
        h.profile(False)
        for k, (t, n) in h.profile_report().items():
            t0, n0 = rep.get(k, (0.0, 0))
            rep[k] = (t0 + t, n0 + n)
    launches = sum(n for _, n in rep.values())
    kernel_ms = sum(t for t, _ in rep.values())
    mg = sum(n for k, (_, n) in rep.items() if k.startswith("k_mg_"))
    cf = rep.get("k_phi_cf_bc", (0.0, 0))
    out = dict(base=a.base, numerics=a.numerics, levels=len(r.lev), zones_per_level=[lev.boxes[0].n for lev in r.lev],
               steps_per_window=a.steps, ms_per_coarse_step={k: dict(median=_median(v), min=min(v), max=max(v)) for k, v in ms.items()},
               cycles_last_solves=cycles, launches_per_coarse_step=launches, multigrid_launches=mg, kernel_ms_profiled_step=kernel_ms,
               k_phi_cf_bc=dict(launches=cf[1], ms=cf[0], share_of_launches=cf[1] / float(max(launches, 1)),
                                share_of_kernel_time=cf[0] / max(kernel_ms, 1e-300)),
               top_kernels=sorted(((k, t, n) for k, (t, n) in rep.items()), key=lambda x: -x[1])[:8])
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    for x in runs.values():
        x.close()


if __name__ == "__main__":
    main()

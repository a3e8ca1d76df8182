#!/usr/bin/env python3
"""What castro.update_sources_after_reflux costs (CastroAmr(update_sources_after_reflux=True)): SURVEY.md config 4 + constant
gravity -- Sedov 128^3 base, two tag-driven refined levels of Berger-Rigoutsos boxes, subcycled, regrid_int 2, from a developed
blast wave (the configuration of tools/amr_bench.py 128 <steps> 2 cluster 0.005 eff=0.7 grav=-1.0) -- with the option off and
on in ONE process on one GPU: the two hierarchies are evolved to the same time and then stepped in alternating blocks, so that
both see the same clocks.  Prints ms per coarse step of either, and -- from two profiled coarse steps of each (the contexts' own
launch counters; they perturb the timing, so they run after it) -- the launches per kernel.

usage: reflux_sources_cost.py [steps per block = 10] [blocks = 3] [t_start = 0.005] [eff=0.7] [grav=-1.0] [only=off|on]
`only`: one hierarchy alone, no timing comparison (also runs on a revision without the keyword when only=off): the launch
counters of two coarse steps, for a comparison between revisions.  The build: CASTRO_AMD_NUMERICS."""
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import castro_amd

pos = [a for a in sys.argv[1:] if "=" not in a]
kw = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
steps = int(pos[0]) if len(pos) > 0 else 10
blocks = int(pos[1]) if len(pos) > 1 else 3
t_start = float(pos[2]) if len(pos) > 2 else 0.005
only = kw.get("only")


def make(option):
    extra = {"update_sources_after_reflux": True} if option else {}     # off: the call a revision without the keyword takes too
    a = castro_amd.CastroAmr((128, 128, 128), refine=[("density", "gradient", 0.05), ("rho_E", "relative_gradient", 0.5)],
                             regrid_int=2, n_error_buf=2, blocking_factor=16, max_level=2, cluster=True,
                             grid_eff=float(kw.get("eff", 0.7)), max_grid_size=128, do_grav=True, const_grav=float(kw.get("grav", -1.0)),
                             **extra)
    a.initData("sedov")
    a.evolve(t_start)
    for _ in range(3):
        a.step()
    torch.cuda.synchronize()
    return a


def block(a, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        a.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def launches(a):
    """{kernel: launches} of regrid_int = 2 consecutive coarse steps (one regrid cycle), over every context of the hierarchy"""
    for h in a.all_hydros():
        h.profile(True)
        h.profile_reset()
    for _ in range(2):
        a.step()
    torch.cuda.synchronize()
    out = {}
    for h in a.all_hydros():
        for name, (ms, n) in h.profile_report().items():
            out[name] = out.get(name, 0) + int(n)
        h.profile(False)
    return dict(sorted(out.items()))


names = [n for n in ("off", "on") if only in (None, n)]
runs = {n: make(n == "on") for n in names}
res = {"workload": "Sedov 128^3 base + 2 tag-driven refined levels (Berger-Rigoutsos boxes), constant gravity, from t = %g" % t_start,
       "numerics": runs[names[0]].lev[0].hydro.numerics, "steps_per_block": steps, "blocks": blocks}
if only is None:
    ms = {n: [] for n in names}
    for _ in range(blocks):
        for n in names:
            ms[n].append(block(runs[n], steps))
    for n in names:
        res["ms_per_coarse_step_" + n] = [round(x, 2) for x in ms[n]]
for n in names:
    a = runs[n]
    res["boxes_per_level_" + n] = [len(lev.boxes) for lev in a.levels]
    cnt = launches(a)
    res["launches_" + n] = cnt
    res["launches_total_" + n] = sum(cnt.values())
print(json.dumps(res))

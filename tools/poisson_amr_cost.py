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

    python tools/poisson_amr_cost.py [--base 64] [--steps 3] [--reps 3] [--numerics contract] [--out file.json] [--clustered]

--clustered: the same problem with tagged, clustered grids instead (a density-gradient tag, cluster=True, max_grid_size = 32 zones
of the new level, the smallest blocking factor of 8, 16, 32 the bottom solver accepts; --r0, the radius of the ball, keeps the
tagged shell off the domain boundary): every refined level is a union of several boxes, solved as ONE array over their bounding
box BB with a coverage mask (k_mgb_*).  After two coarse steps, for every such level: the masked solve from phi = 0 with the
level's own density and boundary values, beside the one-box solve of BB (what a level of one bounding box costs: the same
entry points the parent revision has; its density is the level's, the ambient value where no box is) -- ms per solve and per
V-cycle over --reps repeats (median, min, max), the cycles, and the covered fraction of BB.  A hierarchy of hundreds of boxes is
made and stepped box by box on the host: the default --base of this leg, 32, keeps that to seconds.
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


def _stats(v):
    return dict(median=_median(v), min=min(v), max=max(v))


def clustered_leg(a):
    """the masked solve of every refined level of several boxes beside the one-box solve of its bounding box"""
    import math
    import torch
    import castro_amd
    from castro_amd import _lib
    amr, err = None, None
    for bf in (8, 16, 32):
        try:
            amr = castro_amd.CastroAmr((a.base,) * 3, params=_lib.default_params(**PARAMS), do_grav=True, max_level=2, cluster=True,
                                       refine=[("density", "gradient", 1.e8)], max_grid_size=32, blocking_factor=bf, regrid_int=2,
                                       make_hydro=lambda: castro_amd.HipHydro(0, numerics=a.numerics),
                                       gravity=castro_amd.PoissonGravity(center=CENTER), **GEOM)
            amr.initData("dust_collapse", **dict(PROB, r_0=a.r0))
            break
        except (ValueError, NotImplementedError) as e:      # the bottom limit of a union, a box on the domain boundary
            amr, err = None, "blocking_factor %d: %s" % (bf, e)
    if amr is None:
        sys.exit("no hierarchy the level solves accept: " + err)
    print("hierarchy: blocking_factor %d, boxes per level %s" % (bf, [len(lev.boxes) for lev in amr.lev]), file=sys.stderr, flush=True)
    for _ in range(2):
        amr.step()
    torch.cuda.synchronize()
    print("two coarse steps made", file=sys.stderr, flush=True)
    g, fourpiG = amr.gravity, 4.0 * math.pi * amr.gravity.Gconst
    levels = []
    for l in range(1, len(amr.lev)):
        lev, ent, par = amr.lev[l], g._entry(l), g._entry(l - 1)
        if ent["boxes"] is None:
            levels.append(dict(level=l, boxes=1, note="one box: nothing to compare"))
            continue
        h, bb, pbx = lev.hydro, ent["bb"], ent["phibox"]
        n = tuple(bb[1][d] - bb[0][d] + 1 for d in range(3))
        covered = sum(b.n[0] * b.n[1] * b.n[2] for b in lev.mine)
        plan = g.plan_level(l)
        rhos = [(b.S_new_b, b.gbox) for b in lev.mine]
        h.poisson_boxes_cf_bc(plan, ent["faces"], ent["facebox"], par["phi_old"], par["phibox"], par["phi_new"], par["phibox"], 1.0)
        # the bounding box as ONE box: its density gathered from the boxes, the ambient value elsewhere
        geom = _lib.Geom.from_buffer_copy(lev.geom)
        for d in range(3):
            geom.domlo[d], geom.domhi[d], geom.lo_bc[d], geom.hi_bc[d] = bb[0][d], bb[1][d], 2, 2
        oplan = h.poisson_plan_create(geom)
        U = h.alloc(1, *bb)
        U.fill_(PROB["rho_ambient"])
        sl = lambda box, lo, hi: tuple(slice(lo[d] - box[0][d], hi[d] - box[0][d] + 1) for d in (2, 1, 0))
        for b in lev.mine:
            U[0][sl(bb, b.lo, b.hi)] = b.S_new_b[_lib.URHO][sl(b.gbox, b.lo, b.hi)]
        phi, one = h.alloc(1, *pbx), h.alloc(1, *pbx)
        t = {"masked": [], "one_box": []}
        cyc = {}
        for rep in range(a.reps + 1):                            # the first repeat warms up and is dropped
            for k in ("masked", "one_box"):                      # alternating: a drift of the machine meets both alike
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if k == "masked":
                    phi.zero_()
                    out = h.poisson_boxes_solve(plan, phi, pbx, ent["faces"], ent["facebox"], rhos, _lib.URHO, fourpiG,
                                                g.reltol, g.abstol, g.maxiter)
                else:
                    one.zero_()
                    h.poisson_cf_bc(one, pbx, bb[0], bb[1], par["phi_old"], par["phibox"], par["phi_new"], par["phibox"], 1.0)
                    out = h.poisson_solve(oplan, one, pbx, U, bb, 0, fourpiG, g.reltol, g.abstol, g.maxiter)
                torch.cuda.synchronize()
                if rep > 0:
                    t[k].append((time.perf_counter() - t0) * 1e3)
                cyc[k] = (out[0], bool(out[1]))
        h.poisson_plan_destroy(oplan)
        levels.append(dict(level=l, boxes=len(lev.mine), bounding_box=bb, zones_of_bb=n[0] * n[1] * n[2], covered_fraction=covered / float(n[0] * n[1] * n[2]),
                           multigrid_levels=dict(masked=len(_lib.poisson_boxes_levels(ent["boxes"])), one_box=len(_lib.poisson_level_extents(n))),
                           cycles={k: v[0] for k, v in cyc.items()}, converged={k: v[1] for k, v in cyc.items()},
                           ms_per_solve={k: _stats(v) for k, v in t.items()},
                           ms_per_vcycle={k: _stats([x / max(cyc[k][0], 1) for x in v]) for k, v in t.items()}))
    out = dict(leg="clustered", base=a.base, numerics=a.numerics, r0=a.r0, blocking_factor=bf, max_grid_size=32, reps=a.reps,
               boxes_per_level=[len(lev.boxes) for lev in amr.lev], levels=levels)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    amr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clustered", action="store_true")
    ap.add_argument("--r0", type=float, default=3.0e8)
    ap.add_argument("--base", type=int, default=None, help="zones per direction of level 0: 64, with --clustered 32")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.base is None:
        a.base = 32 if a.clustered else 64
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/poisson_amr_cost.py measures on a GPU; there is none")
    if a.clustered:
        return clustered_leg(a)
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

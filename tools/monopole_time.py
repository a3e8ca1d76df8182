#!/usr/bin/env python
"""Cost of one monopole gravity construction on one MI355X: hipEvent times of castro_amd_radial_mass_mf (k_radial_partial +
k_radial_final), castro_amd_radial_gravity and castro_amd_monopole_grav_fab, for gravity.drdxfac 1 and 4, and, in the same
process on the same state, of castro_amd_estdt_mf as the streaming yardstick.  Warm-up, then the median of --reps timings.

    python tools/monopole_time.py [--sizes 256] [--drdxfac 1 4] [--reps 20] [--numerics contract] [--out file.json]

--amr: instead, the dust-collapse hierarchy (Exec/gravity_tests/DustCollapse octant, base 16^3 + a fixed 16^3 fine patch, drdxfac 2)
with CastroAmr(gravity=MonopoleGravity(...)): wall time per coarse step (synchronised, median of --reps steps after 3 warm-up
steps) with the gravity sources in the one-pass kernel and as separate calls (CASTRO_AMD_SOURCES_ONE_PASS=0), and the hipEvent
time of the radial-mass call of every level.  No threshold is set anywhere.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.diag_time import timed  # noqa: E402


def amr_leg(a):
    import statistics
    import time
    import torch
    import castro_amd
    from castro_amd import _lib as L
    geom = dict(prob_lo=(0., 0., 0.), prob_hi=(7.5e8, 7.5e8, 7.5e8), lo_bc=(3, 3, 3), hi_bc=(2, 2, 2))
    prob = dict(rho_0=1.e9, r_0=6.5e8, p_0=1.e15, rho_ambient=1.0e-5, smooth_delta=4.e6, nsub=5)
    params = dict(eos_gamma=1.66666, small_dens=1.e-6, small_temp=1.e-3, cfl=0.5, init_shrink=0.1, change_max=1.05)
    res = dict(device=torch.cuda.get_device_name(0), numerics=a.numerics, reps=a.reps, amr={})
    for form in ("one_pass", "separate"):
        os.environ["CASTRO_AMD_SOURCES_ONE_PASS"] = "1" if form == "one_pass" else "0"
        g = castro_amd.MonopoleGravity(drdxfac=2, center=(0., 0., 0.))
        amr = castro_amd.CastroAmr((16, 16, 16), patch_crse=((0, 0, 0), (7, 7, 7)), params=L.default_params(**params),
                                   make_hydro=lambda: castro_amd.HipHydro(0, numerics=a.numerics), do_grav=True, gravity=g, **geom)
        amr.initData("dust_collapse", **prob)
        for _ in range(3):
            amr.step()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            amr.step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        res["amr"][form] = dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts))
        print("AMR dust collapse, %s: %.3f ms per coarse step (min %.3f, max %.3f)" % (form, statistics.median(ts), min(ts), max(ts)))
        if form == "one_pass":
            for l, lev in enumerate(amr.lev):
                h, ent = lev.hydro, g._arrays(l)
                box = h.make_diag_boxes([(b.lo, b.hi, (b.S_new_b, b.gbox), None) for b in lev.mine])
                med, lo, hi = timed(lambda: h.radial_mass_mf(box, lev.geom, g.params(l), ent["mv"]), a.reps)
                res["amr"]["radial_mass_level_%d" % l] = dict(ms_median=med, ms_min=lo, ms_max=hi, n1d=g.n1d(l))
                print("  radial_mass_mf level %d (n1d %d): %.4f ms" % (l, g.n1d(l), med))
    os.environ.pop("CASTRO_AMD_SOURCES_ONE_PASS", None)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--amr", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[256])
    ap.add_argument("--drdxfac", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "the median of at least 20 timings"
    import torch
    import castro_amd
    from castro_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("monopole_time.py measures on the GPU; there is nothing to time without one")
    if a.amr:
        return amr_leg(a)
    res = dict(device=torch.cuda.get_device_name(0), numerics=a.numerics, reps=a.reps, sizes=[])
    for n in a.sizes:
        c = castro_amd.Castro((n, n, n), numerics=a.numerics)
        c.initData("sedov", r_init=0.05, nsub=4)
        h, S = c.hydro, c.S_new_b
        dbox = h.make_diag_boxes([(c.lo, c.hi, (S, c.gbox), None)])
        sbox = h.make_state_boxes([(c.lo, c.hi, (S, c.gbox))])
        red = torch.full((3,), 1.e200, dtype=torch.float64, device=S.device)
        gbox = (tuple(x - 1 for x in c.lo), tuple(x + 1 for x in c.hi))
        grav = h.alloc(3, *gbox)
        row = dict(n=n)
        med, lo, hi = timed(lambda: h.estdt_cfl_mf(sbox, c.geom, c.params, red), a.reps)
        row["estdt_mf"] = dict(ms_median=med, ms_min=lo, ms_max=hi)
        for f in a.drdxfac:
            mono = L.make_monopole(c.n_cell, c.geom, (0.5, 0.5, 0.5), f)
            mv = torch.zeros(2 * mono.n1d, dtype=torch.float64, device=S.device)
            rg = torch.zeros(mono.n1d, dtype=torch.float64, device=S.device)
            parts = {}
            for name, fn in (("radial_mass_mf", lambda: h.radial_mass_mf(dbox, c.geom, mono, mv)),
                             ("radial_gravity", lambda: h.radial_gravity(mono, c.geom, mv, rg)),
                             ("monopole_grav_fab", lambda: h.monopole_grav(rg, mono, c.geom, grav, gbox))):
                med, lo, hi = timed(fn, a.reps)
                parts[name] = dict(ms_median=med, ms_min=lo, ms_max=hi)
            total = sum(p["ms_median"] for p in parts.values())
            parts.update(n1d=mono.n1d, total_ms=total, over_estdt=total / row["estdt_mf"]["ms_median"])
            row["drdxfac_%d" % f] = parts
            print("%d^3 drdxfac %d (n1d %d): radial_mass_mf %.4f ms  radial_gravity %.4f ms  monopole_grav_fab %.4f ms  total %.4f ms"
                  "  = %.1f x estdt_mf (%.4f ms)" % (n, f, mono.n1d, parts["radial_mass_mf"]["ms_median"],
                                                     parts["radial_gravity"]["ms_median"], parts["monopole_grav_fab"]["ms_median"],
                                                     total, parts["over_estdt"], row["estdt_mf"]["ms_median"]))
        res["sizes"].append(row)
        c.close()
        del c, S, dbox, sbox, grav
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

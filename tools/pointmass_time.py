#!/usr/bin/env python
"""Cost of the central point mass on one MI355X: hipEvent times of castro_amd_add_pointmass_fab over the (n + 2)^3 gravity FAB
of an n^3 box -- one call per gravity construction, a read-modify-write of 24 B per zone, printed next to that byte floor --
and of the castro_amd_pointmass_delta_mf + castro_amd_pointmass_apply_mf pair of Castro::pointmass_update (64 zones: launch
latency).  Warm-up, then the median of --reps timings; no threshold is set anywhere.

    python tools/pointmass_time.py [--sizes 256] [--reps 20] [--numerics contract] [--out file.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.diag_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "the median of at least 20 timings"
    import torch
    import castro_amd
    from castro_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("pointmass_time.py measures on the GPU; there is nothing to time without one")
    res = dict(device=torch.cuda.get_device_name(0), numerics=a.numerics, reps=a.reps, sizes=[])
    for n in a.sizes:
        c = castro_amd.Castro((n, n, n), numerics=a.numerics, do_grav=True, const_grav=-1.0, use_point_mass=True, point_mass=1.e-3,
                              Gconst=1.0, point_mass_fix_solution=True)
        c.initData("sedov", r_init=0.05, nsub=4)
        c.step()
        h, pm = c.hydro, c.pm
        par = pm.params([0.5, 0.5, 0.5])
        nbytes = 24.0 * (n + 2) ** 3
        row = dict(n=n, bytes=nbytes)
        med, lo, hi = timed(lambda: h.add_pointmass(c.grav_new, c.gravbox, par, c.geom, pm.mass), a.reps)
        row["add_pointmass"] = dict(ms_median=med, ms_min=lo, ms_max=hi, GBps=nbytes / med * 1e-6)
        tab = h.make_pointmass_boxes([(c.lo, c.hi, (c.S_old_b, c.gbox), (c.S_new_b, c.gbox))])

        def pair():
            h.pointmass_delta_mf(tab, par, c.geom, pm.delta)
            h.pointmass_apply_mf(tab, par, c.geom, pm.delta, pm.mass)
        med, lo, hi = timed(pair, a.reps)
        row["delta_apply"] = dict(ms_median=med, ms_min=lo, ms_max=hi)
        print("%d^3 (%s): k_add_pointmass %.4f ms (min %.4f max %.4f), %.3f GB moved at least: %.0f GB/s;  delta + apply %.4f ms "
              "(min %.4f max %.4f)" % (n, a.numerics, row["add_pointmass"]["ms_median"], row["add_pointmass"]["ms_min"],
                                       row["add_pointmass"]["ms_max"], nbytes * 1e-9, row["add_pointmass"]["GBps"],
                                       row["delta_apply"]["ms_median"], row["delta_apply"]["ms_min"], row["delta_apply"]["ms_max"]))
        res["sizes"].append(row)
        c.close()
        del c, tab
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

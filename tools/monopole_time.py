#!/usr/bin/env python
"""Cost of one monopole gravity construction on one MI355X: hipEvent times of castro_amd_radial_mass_mf (k_radial_partial +
k_radial_final), castro_amd_radial_gravity and castro_amd_monopole_grav_fab, for gravity.drdxfac 1 and 4, and, in the same
process on the same state, of castro_amd_estdt_mf as the streaming yardstick.  Warm-up, then the median of --reps timings.

    python tools/monopole_time.py [--sizes 256] [--drdxfac 1 4] [--reps 20] [--numerics contract] [--out file.json]
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

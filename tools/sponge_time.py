#!/usr/bin/env python
"""Cost of the sponge inside the one-pass new-time source kernel on one MI355X: hipEvent times of the stage-1 call of
castro_amd_sources_mf (Sedov state, constant gravity) without and with a sponge (castro_amd_sources_mf_opts), and of the
separate castro_amd_new_sponge_source_fab call.  The sponge reads and writes nothing the kernel does not move already, so the
difference is what its sqrt, cos and divisions cost.  Warm-up, then the median of --reps timings; no threshold is set anywhere.

    python tools/sponge_time.py [--sizes 256] [--reps 20] [--numerics contract] [--out file.json]
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
        sys.exit("sponge_time.py measures on the GPU; there is nothing to time without one")
    res = dict(device=torch.cuda.get_device_name(0), numerics=a.numerics, reps=a.reps, sizes=[])
    for n in a.sizes:
        # the radial ramp lies across the blast, the density and the pressure ramp are off: one sqrt and, in the ramp, one cos
        sp = L.make_sponge(1.e-3, lower_radius=0.1, upper_radius=0.4, center=(0.5, 0.5, 0.5))
        c = castro_amd.Castro((n, n, n), numerics=a.numerics, do_grav=True, const_grav=-1.0, sponge=sp)
        c.initData("sedov", r_init=0.05, nsub=4)
        c.step()                                  # fills the mass fluxes the gravity source reads
        h, dt = c.hydro, c.dt
        boxes = h.make_source_boxes([c._source_spec(1)])
        keep = c.S_new_b.clone()
        row = dict(n=n)
        for name, kw in (("sources_new", {}), ("sources_new_sponge", {"sponge": sp})):
            # every launch applies dt * source to S_new once more; ntimes=1 keeps the state physical, and the time of the
            # kernel does not depend on the values
            med, lo, hi = timed(lambda: h.sources_mf(1, boxes, c.grav, c.grav_source_type, None, c.geom, c.params, dt, ntimes=1, **kw),
                                a.reps)
            c.S_new_b.copy_(keep)
            row[name] = dict(ms_median=med, ms_min=lo, ms_max=hi)
        med, lo, hi = timed(lambda: h.new_sponge_source(c.S_new_b, c.gbox, c.new_source, c.bx, c.lo, c.hi, sp, c.geom, c.params, dt),
                            a.reps)
        row["new_sponge_source_fab"] = dict(ms_median=med, ms_min=lo, ms_max=hi)
        row["sponge_extra_ms"] = row["sources_new_sponge"]["ms_median"] - row["sources_new"]["ms_median"]
        print("%d^3 (%s): k_sources_new %.4f ms (min %.4f max %.4f)  with sponge %.4f ms (min %.4f max %.4f)  difference %.4f ms;"
              "  separate k_new_sponge_source %.4f ms"
              % (n, a.numerics, row["sources_new"]["ms_median"], row["sources_new"]["ms_min"], row["sources_new"]["ms_max"],
                 row["sources_new_sponge"]["ms_median"], row["sources_new_sponge"]["ms_min"], row["sources_new_sponge"]["ms_max"],
                 row["sponge_extra_ms"], row["new_sponge_source_fab"]["ms_median"]))
        res["sizes"].append(row)
        c.close()
        del c, boxes, keep
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Cost of the integrated quantities on one MI355X: hipEvent times of castro_amd_integrated_quantities_mf (k_diag_partial +
k_diag_final: 7 state planes read per zone) and, in the same process on the same state, of castro_amd_estdt_mf (k_estdt: 5 planes)
as the streaming yardstick.  Warm-up, then the median of --reps timings per size; TB/s over the compulsory bytes.

    python tools/diag_time.py [--sizes 256 128] [--reps 30] [--numerics contract] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 128])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "the median of at least 20 timings"
    import torch
    import castro_amd
    from castro_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("diag_time.py measures on the GPU; there is nothing to time without one")
    res = dict(device=torch.cuda.get_device_name(0), numerics=a.numerics, reps=a.reps, sizes=[])
    for n in a.sizes:
        c = castro_amd.Castro((n, n, n), numerics=a.numerics)
        c.initData("sedov", r_init=0.05, nsub=4)
        h, S = c.hydro, c.S_new_b
        dbox = h.make_diag_boxes([(c.lo, c.hi, (S, c.gbox), None)])
        sbox = h.make_state_boxes([(c.lo, c.hi, (S, c.gbox))])
        out = torch.zeros(L.DIAG_N, dtype=torch.float64, device=S.device)
        red = torch.full((3,), 1.e200, dtype=torch.float64, device=S.device)
        center = [0.5, 0.5, 0.5]
        zones = float(n) ** 3
        row = dict(n=n, workgroups=h.diag_workgroups(dbox))
        for name, planes, fn in (("integrated_quantities_mf", 7, lambda: h.integrated_quantities_mf(dbox, c.geom, center, out)),
                                 ("estdt_mf", 5, lambda: h.estdt_cfl_mf(sbox, c.geom, c.params, red))):
            med, lo, hi = timed(fn, a.reps)
            row[name] = dict(ms_median=med, ms_min=lo, ms_max=hi, planes=planes, bytes=planes * 8.0 * zones,
                             tb_per_s=planes * 8.0 * zones / (med * 1e-3) / 1e12)
        row["diag_over_estdt_bytes_per_s"] = row["integrated_quantities_mf"]["tb_per_s"] / row["estdt_mf"]["tb_per_s"]
        res["sizes"].append(row)
        print("%d^3: integrated_quantities_mf %.4f ms (%.2f TB/s, %d workgroups)   estdt_mf %.4f ms (%.2f TB/s)   ratio of bytes/s %.2f"
              % (n, row["integrated_quantities_mf"]["ms_median"], row["integrated_quantities_mf"]["tb_per_s"], row["workgroups"],
                 row["estdt_mf"]["ms_median"], row["estdt_mf"]["tb_per_s"], row["diag_over_estdt_bytes_per_s"]))
        c.close()
        del c, S, dbox, sbox
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

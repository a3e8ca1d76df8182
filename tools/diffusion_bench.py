#!/usr/bin/env python
"""Streaming rate of the thermal-diffusion kernels against the project's own yardstick, k_ctoprim, in one process.

  python tools/diffusion_bench.py [--n 256] [--reps 20] [--numerics contract] [--steps 10]

Times with hipEvents (the context's per-launch profiler), over `reps` repetitions after warm-up on an n^3 box:
  (a) castro_amd_temp_diffusion_fab            compulsory bytes: rho, T read once + two source planes read and written = 48 B / zone
  (b) castro_amd_estdt_temp_diffusion_fab      rho, rho X read once = 16 B / zone
  (c) k_ctoprim of a plain Sedov step          bench.py's plane counts over the ghost-grown box
and the wall time of a Sedov step on the sources path with gravity only against the same step with diffusion as well (the
price of the second stencil launch per stage and of the ghost fill of S_new).  Prints one JSON line."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stamp():
    h = hashlib.sha1()
    d = os.path.join(ROOT, "castro_amd", "csrc")
    for f in ("hydro_device.h", "ctu_kernels.h", "ctu_kernels.hip", "aux_kernels.hip", "diffusion_kernels.hip", "capi.hip"):
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--numerics", default="contract")
    a = ap.parse_args()
    import torch
    import bench
    import castro_amd
    n = (a.n,) * 3
    zones = a.n ** 3
    out = {"box": list(n), "numerics": a.numerics, "reps": a.reps, "stamp": stamp(), "device": torch.cuda.get_device_name(0)}

    def per_launch(h, name):
        rep = h.profile_report()
        ms, cnt = rep[name]
        return ms / cnt, cnt

    # ---- (c) the yardstick: k_ctoprim of a plain step, and (a), (b) on the state it leaves
    c = castro_amd.Castro(n, numerics=a.numerics)
    c.initData("sedov", r_init=0.05, nsub=4)
    for _ in range(3):
        c.step()
    h = c.hydro
    h.profile(True)
    h.profile_reset()
    for _ in range(a.reps):
        c.step()
    torch.cuda.synchronize()
    name = max((k for k in h.profile_report() if k.startswith("k_ctoprim")), key=lambda k: h.profile_report()[k][1])
    ms, cnt = per_launch(h, name)
    lean = a.numerics == "contract"
    nbytes = bench.kernel_bytes_per_unit(name, False, lean) * bench.kernel_units(name, n)
    out["ctoprim"] = {"kernel": name, "launches": cnt, "ms": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6}

    diff = castro_amd.make_diffusion(1.e3)
    src = h.alloc(7, c.lo, c.hi)
    red = torch.full((1,), 1.e300, dtype=torch.float64, device="cuda")
    for _ in range(3):                                                   # warm-up
        h.temp_diffusion(c.S_new_b, c.gbox, src, c.bx, c.lo, c.hi, diff, c.geom, 1.0)
        h.estdt_temp_diffusion(c.S_new_b, c.gbox, c.lo, c.hi, c.geom, c.params, diff, 1.e200, red)
    torch.cuda.synchronize()
    h.profile_reset()
    for _ in range(a.reps):
        h.temp_diffusion(c.S_new_b, c.gbox, src, c.bx, c.lo, c.hi, diff, c.geom, 1.0)
        h.estdt_temp_diffusion(c.S_new_b, c.gbox, c.lo, c.hi, c.geom, c.params, diff, 1.e200, red)
    torch.cuda.synchronize()
    for key, kname, bpz in (("temp_diffusion", "k_temp_diffusion", 48), ("estdt_temp_diffusion", "k_estdt_temp_diffusion", 16)):
        ms, cnt = per_launch(h, kname)
        out[key] = {"kernel": kname, "launches": cnt, "ms": ms, "bytes": bpz * zones, "GBps": bpz * zones / ms / 1e6}
    out["temp_diffusion"]["rate_over_ctoprim"] = out["temp_diffusion"]["GBps"] / out["ctoprim"]["GBps"]
    h.profile(False)
    c.close()
    del c, src

    # ---- a Sedov step on the sources path: gravity only against gravity + diffusion
    for key, kw in (("step_gravity_ms", {}), ("step_gravity_diffusion_ms", {"diffusion": diff})):
        c = castro_amd.Castro(n, numerics=a.numerics, do_grav=True, const_grav=-0.5, **kw)
        c.initData("sedov", r_init=0.05, nsub=4)
        for _ in range(3):
            c.step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            c.step()
        e1.record()
        torch.cuda.synchronize()
        out[key] = e0.elapsed_time(e1) / a.steps
        c.hydro.profile(True)
        c.step()
        torch.cuda.synchronize()
        out[key.replace("_ms", "_kernels_ms")] = {k: round(v[0] / v[1], 4) for k, v in c.hydro.profile_report().items()
                                                  if k.startswith(("k_sources", "k_temp_diff", "k_estdt", "k_pack", "k_unpack", "k_bc_fill"))}
        c.close()
        del c
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Cost of the boundary overrides of the state fill on one MI355X.

Kernels: hipEvent times of castro_amd_ext_bc_fill_fab on the 264^3 state FAB of a 256^3 box -- k_hse_fill for a z-low and for an
x-low face (on z low the lanes of a wave run along x, unit stride; on x low they are a row apart), k_ambient_fill for the same
two faces -- beside castro_amd_bc_fill_fab (k_bc_fill) on the same FAB.  Warm-up, then the median of --reps timings.

Step: an isothermal atmosphere under constant gravity at 256^3, z low Inflow; the wall time per step of --steps steps after a
warm-up, without ext_bc, with ext_bc = make_ext_bc(zl="hse") and with an ext_bc that overrides nothing (the price of the option
itself), each run --runs times: the spread of the runs without ext_bc is the yardstick for the difference.  With --plain-only the tool needs nothing this feature added, so the same script times the step
of an older revision.  No threshold is set anywhere.

    python tools/ext_bc_time.py [--n 256] [--reps 20] [--steps 20] [--runs 5] [--numerics contract] [--plain-only] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.diag_time import timed  # noqa: E402


def atmosphere(c, n, H=0.25, g=-1.0):
    import torch
    z = (torch.arange(n, dtype=torch.float64, device="cuda") + 0.5) / n
    S = torch.zeros((8, n, n, n), dtype=torch.float64, device="cuda")
    S[0] = torch.exp(-z / H)[:, None, None]
    S[4] = S[5] = S[0] * (-g * H) / (c.params.eos_gamma - 1.0)
    S[6], S[7] = 1.0, S[0]
    c.set_state(S)


def step_ms(castro_amd, n, numerics, ext, steps, warmup=4):
    import torch
    kw = {} if ext is None else {"ext_bc": ext}
    c = castro_amd.Castro((n, n, n), numerics=numerics, do_grav=True, const_grav=-1.0, lo_bc=(4, 4, 1), hi_bc=(4, 4, 3), **kw)
    atmosphere(c, n)
    for _ in range(warmup):
        c.step(1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        c.step(1.0)
    torch.cuda.synchronize()
    ms = 1.e3 * (time.perf_counter() - t0) / steps
    c.close()
    del c
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "the median of at least 20 timings"
    import torch
    import castro_amd
    from castro_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("ext_bc_time.py measures on the GPU; there is nothing to time without one")
    n = a.n
    res = dict(device=torch.cuda.get_device_name(0), numerics=a.numerics, n=n, reps=a.reps, steps=a.steps, kernels={}, step={})
    if not a.plain_only:
        h = castro_amd.HipHydro(0, numerics=a.numerics)
        P = L.default_params()
        box = ((-4, -4, -4), (n + 3, n + 3, n + 3))
        U = h.alloc(8, *box, fill=1.0)
        U[6] = 1.e-8
        for face, d in (("z_low", 2), ("x_low", 0)):
            lo_bc, hi_bc = [4, 4, 4], [4, 4, 4]
            for kind, bc in (("hse", 1), ("ambient", 2)):
                lo_bc[d] = bc
                geom = L.make_geom((n, n, n), lo_bc=lo_bc, hi_bc=hi_bc)
                ext = L.make_ext_bc(**({"xz"[d == 2] + "l": "hse"} if kind == "hse" else dict(fill_ambient_bc=1, ambient_fill_dir=d)))
                ext = L.complete_ext_bc(ext, P, -1.0)
                if kind == "hse":
                    key = "bc_fill_%s" % face
                    res["kernels"][key] = dict(zip(("ms_median", "ms_min", "ms_max"), timed(lambda: h.bc_fill(U, box, geom), a.reps)))
                key = "%s_%s" % (kind, face)
                res["kernels"][key] = dict(zip(("ms_median", "ms_min", "ms_max"),
                                               timed(lambda: h.ext_bc_fill(U, box, geom, P, ext), a.reps)))
        for k, v in res["kernels"].items():
            print("%d^3 (%s) %-18s %.4f ms (min %.4f max %.4f)" % (n, a.numerics, k, v["ms_median"], v["ms_min"], v["ms_max"]))
        h.close()
        del U
        torch.cuda.empty_cache()
    # ext_bc_idle: an ext_bc that overrides nothing -- what the option costs by itself (the boundary fill outside the hydro call,
    # the separate clean of Sborder, one call that launches nothing) apart from the walk
    forms = [("plain", None)] + ([] if a.plain_only else [("hse_z_low", L.make_ext_bc(zl="hse")), ("ext_bc_idle", L.make_ext_bc())])
    for name, ext in forms:
        ms = [step_ms(castro_amd, n, a.numerics, ext, a.steps) for _ in range(a.runs)]
        res["step"][name] = dict(ms_per_step=ms, median=statistics.median(ms), spread=max(ms) - min(ms))
        print("%d^3 (%s) step with gravity, %-10s median %.3f ms, runs %s" % (n, a.numerics, name, statistics.median(ms),
                                                                          " ".join("%.3f" % x for x in ms)))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

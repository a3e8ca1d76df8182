#!/usr/bin/env python
"""What a checkpoint costs on one MI355X (castro_amd/checkpoint.py).  Four legs, no threshold anywhere:

  plain   the step time of a source tree that may have no checkpoint at all: Castro 256^3 Sedov, windows of --steps host-free
          steps through run_steps, --reps of them, nothing else.  --root DIR takes the package from DIR instead of this tree
          (a built checkout of the parent commit), so that one session can alternate processes of the two trees and set the
          windows of the `sedov` leg against the parent's.  Uses nothing the parent lacks.

  sedov   Castro 256^3 Sedov, host-free steps.  A window is --steps steps through run_steps and ends in a device synchronise;
          windows without a checkpoint, with a synchronous writeCheckpoint in the middle and with writeCheckpoint(background=True)
          in the middle are timed in alternation, --reps of each.  Reported: the median window of each kind, per step and as the
          time the checkpoint adds to the window -- against the steps of the same session without a checkpoint, the parent
          revision having none to compare with --, and for the background form the time checkpoint_wait() still blocks after the
          window (the file write that the steps did not cover).
  pack    the pack launch alone on the state of that run -- with the min / max reduction, without it, and the same copy through
          castro_amd_fab_ops (CASTRO_AMD_OP_COPY) followed by torch.aminmax over the staging buffer, which is what a writer
          without the kernel would do on the device; --launches launches queued back to back between two synchronises.
  amr     the AMR configuration of tools/reflux_sources_cost.py (Sedov 128^3 base, two clustered levels, constant gravity,
          from a developed blast wave): the same three kinds of window per coarse step, --amr-reps of each (a regrid every
          other step scatters these windows).

Checkpoints go to --dir (default: a temporary directory, removed afterwards) and each is deleted once it has been timed.

    python tools/checkpoint_cost.py [--legs sedov pack amr] [--n 256] [--steps 8] [--reps 3] [--amr-reps 9] [--numerics contract] [--dir D] [--out file.json]
    python tools/checkpoint_cost.py --legs plain [--root PARENT_TREE] [--reps 5]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def windows(run, advance, steps, reps, root):
    """{kind: [ms per window]} and [ms checkpoint_wait blocks after a background window]; advance(k): k steps of `run`"""
    import torch
    out, tail = {"none": [], "sync": [], "background": []}, []
    half = steps // 2
    for rep in range(reps):
        for kind in ("none", "sync", "background"):             # alternating: a drift of the machine meets every kind alike
            d = os.path.join(root, "chk_%s_%d" % (kind, rep))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            advance(half)
            if kind != "none":
                run.writeCheckpoint(d, background=kind == "background")
            advance(steps - half)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out[kind].append((t1 - t0) * 1e3)
            if kind == "background":
                run.checkpoint_wait()
                tail.append((time.perf_counter() - t1) * 1e3)
            shutil.rmtree(d, ignore_errors=True)
    return out, tail


def summarise(name, out, tail, steps, nbytes):
    med = {k: _median(v) for k, v in out.items()}
    row = dict(leg=name, steps_per_window=steps, checkpoint_bytes=nbytes, ms_per_step_without=med["none"] / steps,
               window_ms={k: dict(median=med[k], min=min(v), max=max(v)) for k, v in out.items()},
               added_ms_sync=med["sync"] - med["none"], added_ms_background=med["background"] - med["none"],
               wait_after_background_ms=dict(median=_median(tail), min=min(tail), max=max(tail)))
    print("%s: %.3f ms per step without a checkpoint; a synchronous checkpoint adds %.1f ms to the window, a background one %.1f ms "
          "(+ %.1f ms in checkpoint_wait afterwards); %.1f MB per checkpoint"
          % (name, row["ms_per_step_without"], row["added_ms_sync"], row["added_ms_background"], _median(tail), nbytes / 1e6))
    return row


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(d) for f in fs)


def plain_leg(a, res):
    import torch
    import castro_amd
    n = (a.n, a.n, a.n)
    c = castro_amd.Castro(n, numerics=a.numerics)
    c.initData("sedov", r_init=0.05, nsub=4)
    c.run_steps(8)
    half, out = a.steps // 2, []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.run_steps(half)
        c.run_steps(a.steps - half)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    res["plain"] = dict(tree=os.path.dirname(os.path.dirname(os.path.abspath(castro_amd.__file__))), steps_per_window=a.steps,
                        window_ms=dict(median=_median(out), min=min(out), max=max(out)), ms_per_step=_median(out) / a.steps)
    print("plain %d^3 (%s): %.3f ms per window of %d steps (%.3f .. %.3f) = %.3f ms per step"
          % (a.n, a.root or "this tree", _median(out), a.steps, min(out), max(out), _median(out) / a.steps))
    c.close()


def sedov_leg(a, res, root):
    import torch
    import castro_amd
    n = (a.n, a.n, a.n)
    c = castro_amd.Castro(n, numerics=a.numerics)
    c.initData("sedov", r_init=0.05, nsub=4)
    c.run_steps(8)
    d = c.writeCheckpoint(os.path.join(root, "warm"))           # the staging buffers are allocated here, not in a window
    nbytes = _dir_bytes(d)
    shutil.rmtree(d)
    c.writeCheckpoint(os.path.join(root, "warm"), background=True)
    c.checkpoint_wait()
    shutil.rmtree(os.path.join(root, "warm"))
    out, tail = windows(c, lambda k: c.run_steps(k), a.steps, a.reps, root)
    res["sedov"] = summarise("sedov %d^3" % a.n, out, tail, a.steps, nbytes)
    if "pack" in a.legs:
        pack_leg(a, res, c)
    c.close()


def pack_leg(a, res, c):
    import torch
    from castro_amd import _lib as L
    h = c.hydro
    spec = [(c.S_new_b, c.gbox, (c.lo, c.hi))]
    entries = h.make_pack_entries(spec)
    _, _, doubles, pairs = entries
    dst = torch.empty(doubles, dtype=torch.float64, device="cuda")
    mm = torch.empty(2 * pairs, dtype=torch.float64, device="cuda")
    view = dst.view(L.NUM_STATE, c.n[2], c.n[1], c.n[0])
    ops = h.make_ops([(L.OP_COPY, 0, L.NUM_STATE, c.lo, c.hi, 0.0, 0.0, (view, c.bx), (c.S_new_b, c.gbox), None)])

    def via_ops():
        h.fab_ops(ops)
        flat = dst.view(L.NUM_STATE, -1)
        return flat.amin(dim=1), flat.amax(dim=1)
    forms = {"pack_minmax": lambda: h.fab_pack(entries, dst, mm), "pack_copy_only": lambda: h.fab_pack(entries, dst),
             "fab_ops_copy": lambda: h.fab_ops(ops), "fab_ops_copy_then_torch_minmax": via_ops}
    rows = {}
    for _ in range(3):
        for f in forms.values():
            f()
    for rep in range(a.reps):
        for name, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                f()
            torch.cuda.synchronize()
            rows.setdefault(name, []).append((time.perf_counter() - t0) / a.launches * 1e3)
    nbytes = 2 * 8 * doubles                                    # read once, written once
    res["pack"] = dict(bytes_moved=nbytes, launches=a.launches,
                       ms={k: dict(median=_median(v), min=min(v), max=max(v)) for k, v in rows.items()},
                       tb_per_s={k: nbytes / (_median(v) * 1e-3) / 1e12 for k, v in rows.items()})
    for k, v in rows.items():
        print("pack %d^3 x 8: %s %.4f ms (%.4f .. %.4f), %.2f TB/s of read + write" % (a.n, k, _median(v), min(v), max(v),
                                                                                      res["pack"]["tb_per_s"][k]))


def amr_leg(a, res, root):
    import torch
    import castro_amd
    amr = castro_amd.CastroAmr((128, 128, 128), refine=[("density", "gradient", 0.05), ("rho_E", "relative_gradient", 0.5)],
                               regrid_int=2, n_error_buf=2, blocking_factor=16, max_level=2, cluster=True, grid_eff=0.7,
                               max_grid_size=128, do_grav=True, const_grav=-1.0,
                               make_hydro=lambda: castro_amd.HipHydro(torch.cuda.current_device(), numerics=a.numerics))
    amr.initData("sedov")
    amr.evolve(a.t_start)
    for _ in range(3):
        amr.step()
    d = amr.writeCheckpoint(os.path.join(root, "warm"))
    nbytes = _dir_bytes(d)
    shutil.rmtree(d)

    def advance(k):
        for _ in range(k):
            amr.step()
    steps = max(2, a.steps // 2)
    out, tail = windows(amr, advance, steps, a.amr_reps, root)
    res["amr"] = summarise("amr 128^3 + 2 levels", out, tail, steps, nbytes)
    res["amr"]["boxes_per_level"] = [len(lev.boxes) for lev in amr.lev]
    amr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["sedov", "pack", "amr"], choices=["plain", "sedov", "pack", "amr"])
    ap.add_argument("--root", default=None)
    ap.add_argument("--amr-reps", dest="amr_reps", type=int, default=9)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--t-start", dest="t_start", type=float, default=0.005)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit("checkpoint_cost.py measures on the GPU; there is nothing to time without one")
    res = dict(device=torch.cuda.get_device_name(0), numerics=a.numerics)
    root = a.dir or tempfile.mkdtemp(prefix="castro_amd_chk_")
    os.makedirs(root, exist_ok=True)
    try:
        if "plain" in a.legs:
            plain_leg(a, res)
        if "sedov" in a.legs or "pack" in a.legs:
            sedov_leg(a, res, root)
        if "amr" in a.legs:
            amr_leg(a, res, root)
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

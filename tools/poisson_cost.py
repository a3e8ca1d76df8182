#!/usr/bin/env python
"""What Poisson gravity costs on one MI355X (castro_amd/csrc/poisson_kernels.hip, castro_amd/gravity.py).  No threshold anywhere.

For the dust collapse (Exec/gravity_tests/DustCollapse/inputs_3d_poisson_regtest: the full star, Outflow on all six faces) on
--sizes zones per direction:
  solve     ms per solve and V-cycles per solve, from zero (the first solve of a run) and warm-started (from the converged
            potential of the same density), --reps of each; launches per V-cycle counted by the context's profiler in a solve of
            its own (profiling slows the host: its times are not reported)
  bc        ms of the multipole moments plus the boundary fill at lnum 0 and 6, --launches pairs queued back to back between two
            synchronises
  step      ms per step of Castro(poisson=PoissonGravity()) against the same run with gravity_type="monopole", windows of
            --steps steps ending in a device synchronise, alternating, --reps of each
  sphere    (--sphere sizes) the error of phi against the analytic potential of a uniform sphere of radius r_0,
            -G M (3 R^2 - r^2) / (2 R^3) inside and -G M / r outside, M the mass on the grid, for lnum 0: a measurement, not a test

    python tools/poisson_cost.py [--sizes 64 128 256] [--sphere 32 64] [--steps 4] [--reps 3] [--numerics contract] [--out file.json]
"""
import argparse
import json
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

GEOM = dict(prob_lo=(0., 0., 0.), prob_hi=(1.5e9, 1.5e9, 1.5e9), lo_bc=(2, 2, 2), hi_bc=(2, 2, 2))
CENTER = (7.5e8, 7.5e8, 7.5e8)
# nsub: the initial state is made on the host, and its subsampling does not matter to a timing
PROB = dict(rho_0=1.e9, r_0=6.5e8, p_0=1.e15, rho_ambient=1.0e-5, smooth_delta=4.e6, nsub=2)
PARAMS = dict(eos_gamma=1.66666, small_dens=1.e-6, small_temp=1.e-3, cfl=0.5, init_shrink=0.1, change_max=1.05)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def make_run(n, numerics, poisson, lnum=0):
    import castro_amd
    from castro_amd import _lib
    kw = dict(poisson=castro_amd.PoissonGravity(max_multipole_order=lnum)) if poisson else dict(gravity_type="monopole", drdxfac=4)
    c = castro_amd.Castro((n, n, n), params=_lib.default_params(**PARAMS), numerics=numerics, do_grav=True, **GEOM, **kw)
    c.center = CENTER
    c.initData("dust_collapse", **PROB)
    return c


def _phibox(c):
    """the box of the potential: the valid box grown by one zone"""
    return tuple(x - 1 for x in c.lo), tuple(x + 1 for x in c.hi)


def solve_leg(n, numerics, reps):
    import torch
    from castro_amd import _lib
    c = make_run(n, numerics, True)
    h, pg = c.hydro, c.poisson
    S = c.S_new_b
    mp = _lib.make_multipole(c.geom, pg.problem_center(), pg.lnum, pg.Gconst)
    table = h.make_diag_boxes([(c.lo, c.hi, (S, c.gbox), None)])
    mom = torch.zeros(3 * (pg.lnum + 1) ** 2, dtype=torch.float64, device="cuda")
    fourpiG = 4.0 * math.pi * pg.Gconst
    phi, phibox, plan = c.phi_grav(), _phibox(c), pg.plan_level(0)
    h.multipole_moments_mf(table, c.geom, mp, mom)
    h.multipole_phi_bc(phi, phibox, c.geom, mp, mom)

    def solve(zero):
        if zero:
            phi[:, 1:-1, 1:-1, 1:-1] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = h.poisson_solve(plan, phi, phibox, S, c.gbox, _lib.URHO, fourpiG)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    solve(True)                                                 # warm-up: code objects, the plan's first touch of its arrays
    cold = [solve(True) for _ in range(reps)]
    # warm start: the density moved by one step's worth (0.1 %), from the converged potential -- a solve from the very same
    # right-hand side would take no cycle at all
    S[_lib.URHO] *= 1.001
    warm = [solve(False)]
    for _ in range(reps - 1):
        S[_lib.URHO] *= 1.001
        warm.append(solve(False))
    h.profile(True)
    h.profile_reset()
    _, (cycles, ok, norm, hist) = solve(True)
    h.profile(False)
    rep = h.profile_report()
    launches = sum(v[1] for k, v in rep.items() if k.startswith("k_mg_"))
    setup = 1 + 2 + 3                                           # k_mg_rhs, the norm of b, the starting residual and its norm
    levels = _lib.poisson_level_extents((n, n, n))
    return dict(leg="solve", n=n, numerics=numerics, levels=len(levels), coarsest=levels[-1],
                cold_ms=dict(median=_median([t for t, _ in cold]), min=min(t for t, _ in cold), max=max(t for t, _ in cold)),
                cold_cycles=[o[0] for _, o in cold],
                warm_ms=dict(median=_median([t for t, _ in warm]), min=min(t for t, _ in warm), max=max(t for t, _ in warm)),
                warm_cycles=[o[0] for _, o in warm],
                ms_per_cycle_cold=_median([t / max(o[0], 1) for t, o in cold]),
                launches_per_cycle=(launches - setup) / float(cycles), launches_of_a_solve=launches, final_norm=norm,
                tolerance=max(1e-10 * hist[0], 1e-10 * hist[1]))


def bc_leg(n, numerics, launches):
    import torch
    c = make_run(n, numerics, True)
    h, phi, phibox = c.hydro, c.phi_grav(), _phibox(c)
    out = dict(leg="bc", n=n, numerics=numerics, launches=launches)
    for lnum in (0, 6):
        from castro_amd import _lib
        mp = _lib.make_multipole(c.geom, CENTER, lnum)
        table = h.make_diag_boxes([(c.lo, c.hi, (c.S_new_b, c.gbox), None)])
        mom = torch.zeros(3 * (lnum + 1) ** 2, dtype=torch.float64, device="cuda")
        for _ in range(3):
            h.multipole_moments_mf(table, c.geom, mp, mom)
            h.multipole_phi_bc(phi, phibox, c.geom, mp, mom)
        times = {}
        for what in ("moments", "phi_bc", "both"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(launches):
                if what != "phi_bc":
                    h.multipole_moments_mf(table, c.geom, mp, mom)
                if what != "moments":
                    h.multipole_phi_bc(phi, phibox, c.geom, mp, mom)
            torch.cuda.synchronize()
            times[what] = (time.perf_counter() - t0) * 1e3 / launches
        out["lnum%d_ms" % lnum] = times
    return out


def step_leg(n, numerics, steps, reps):
    import torch
    runs = {"poisson": make_run(n, numerics, True), "monopole": make_run(n, numerics, False)}
    for c in runs.values():
        c.step()
        c.step()
    out = {k: [] for k in runs}
    for _ in range(reps):
        for k, c in runs.items():                                # alternating: a drift of the machine meets both alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                c.step()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / steps)
    st = runs["poisson"].poisson_stats()
    return dict(leg="step", n=n, numerics=numerics, steps_per_window=steps,
                ms_per_step={k: dict(median=_median(v), min=min(v), max=max(v)) for k, v in out.items()},
                cycles_last_step=dict(old=st["old"]["cycles"], new=st["new"]["cycles"]))


def sphere_leg(n, numerics):
    import numpy as np
    import torch
    c = make_run(n, numerics, True)
    c.gravity.get_new_grav_vector(0)
    torch.cuda.synchronize()
    phi = c.phi_grav().cpu().numpy()[0, 1:-1, 1:-1, 1:-1]
    rho = c.S_new().cpu().numpy()[0]
    dx = [c.geom.dx[d] for d in range(3)]
    M = float(rho.sum()) * dx[0] * dx[1] * dx[2]
    x = [(np.arange(n) + 0.5) * dx[d] - CENTER[d] for d in range(3)]
    r = np.sqrt(x[0][None, None, :] ** 2 + x[1][None, :, None] ** 2 + x[2][:, None, None] ** 2)
    R0, G = PROB["r_0"], c.poisson.Gconst
    exact = np.where(r < R0, -G * M * (3.0 * R0 * R0 - r * r) / (2.0 * R0 ** 3), -G * M / r)
    err = np.abs(phi - exact)
    return dict(leg="sphere", n=n, numerics=numerics, lnum=0, mass_on_grid=M, mass_of_the_sphere=4.0 / 3.0 * math.pi * R0 ** 3 * PROB["rho_0"],
                max_error_over_max_phi=float(err.max() / np.abs(exact).max()),
                l1_error_over_mean_phi=float(err.mean() / np.abs(exact).mean()), cycles=c.poisson_stats()["new"]["cycles"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--sphere", type=int, nargs="*", default=[32, 64])
    ap.add_argument("--legs", nargs="*", default=["solve", "bc", "step", "sphere"])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--numerics", default="contract")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/poisson_cost.py measures on a GPU; there is none")
    rows = []
    for n in a.sizes:
        for leg in a.legs:
            if leg == "solve":
                rows.append(solve_leg(n, a.numerics, a.reps))
            elif leg == "bc":
                rows.append(bc_leg(n, a.numerics, a.launches))
            elif leg == "step":
                rows.append(step_leg(n, a.numerics, a.steps, a.reps))
            if leg != "sphere":
                print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    if "sphere" in a.legs:
        for n in a.sphere:
            rows.append(sphere_leg(n, a.numerics))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

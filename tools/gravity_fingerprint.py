#!/usr/bin/env python
"""Fingerprint of the gravity field of the single-level driver: hashes of what three steps of dust-collapse initial data on 16^3
zones leave behind, for every way castro_amd.Castro constructs a per-zone gravity field.  Public calls only; nothing is compared
here -- two commits (or two builds) agree when their outputs are the same text.

  a  gravity_type="monopole", drdxfac=2, grav_source_type=4        e  a with use_point_mass
  b  gravity_type="monopole", drdxfac=2, grav_source_type=2        f  a with the `center` attribute assigned after construction
  c  poisson=PoissonGravity(max_multipole_order=2)                 g  a with CASTRO_AMD_SOURCES_ONE_PASS=0
  d  constant gravity, use_point_mass, point_mass_fix_solution     h  c with CASTRO_AMD_SOURCES_ONE_PASS=0

One line per configuration: the first 16 hex digits of the SHA-256 of S_new, grav_old, grav_new (whole FABs, ghost zones
included), phi_grav(new=True / False), radial_gravity(), point_mass and the cycle counts and norm histories of poisson_stats();
"-" where the configuration has none.  With --launches (device backend) also the kernel launches of the library in the three
steps, by the context's profiler, in a run of their own.

    python tools/gravity_fingerprint.py [--backend oracle|device] [--numerics exact|contract] [--launches] [--only a c ...]
"""
import argparse
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))

N = (16, 16, 16)
GEOM = dict(prob_lo=(0., 0., 0.), prob_hi=(1.5e9, 1.5e9, 1.5e9), lo_bc=(2, 2, 2), hi_bc=(2, 2, 2))
PROB = dict(rho_0=1.e9, r_0=6.5e8, p_0=1.e15, rho_ambient=1.0e-5, smooth_delta=4.e6, nsub=5)
PARAMS = dict(eos_gamma=1.66666, small_dens=1.e-6, small_temp=1.e-3, cfl=0.5, init_shrink=0.1, change_max=1.05)
OFF_CENTER = (7.0e8, 7.5e8, 8.0e8)
STEPS = 3
MONO = dict(gravity_type="monopole", drdxfac=2)
PM = dict(use_point_mass=True, point_mass=2.0e33)
# name: (keywords of Castro, needs a PoissonGravity, centre assigned after construction, CASTRO_AMD_SOURCES_ONE_PASS)
CONFIGS = {
    "a": (dict(MONO, grav_source_type=4), False, None, None),
    "b": (dict(MONO, grav_source_type=2), False, None, None),
    "c": ({}, True, None, None),
    "d": (dict(PM, const_grav=-1.0e3, point_mass_fix_solution=True), False, None, None),
    "e": (dict(MONO, grav_source_type=4, **PM), False, None, None),
    "f": (dict(MONO, grav_source_type=4), False, OFF_CENTER, None),
    "g": (dict(MONO, grav_source_type=4), False, None, "0"),
    "h": ({}, True, None, "0"),
}


def _digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p)
    return h.hexdigest()[:16]


def _tensor(t):
    return _digest(t.detach().cpu().contiguous().numpy().tobytes())


def make_backend(backend, numerics):
    """(backend, its parameter block)"""
    if backend == "device":
        import castro_amd
        from castro_amd import _lib
        return castro_amd.HipHydro(0, numerics=numerics), _lib.default_params(**PARAMS)
    from oracle import oracle_lib
    oracle_lib.build()
    from poisson_ref import PoissonOracleBackend
    from pointmass_ref import PointMassOracleBackend
    return type("FingerprintOracleBackend", (PoissonOracleBackend, PointMassOracleBackend), {})(), oracle_lib.default_params(**PARAMS)


def run(name, backend, numerics, profile=False):
    import castro_amd
    kw, poisson, center, one_pass = CONFIGS[name]
    if poisson:
        kw = dict(kw, poisson=castro_amd.PoissonGravity(max_multipole_order=2))
    if one_pass is not None:
        os.environ["CASTRO_AMD_SOURCES_ONE_PASS"] = one_pass
    try:
        hydro, params = make_backend(backend, numerics)
        c = castro_amd.Castro(N, params=params, hydro=hydro, do_grav=True, **GEOM, **kw)
        if center is not None:
            c.center = center
        c.initData("dust_collapse", **PROB)
        if profile:
            c.hydro.profile(True)
            c.hydro.profile_reset()
        for _ in range(STEPS):
            c.step()
        if profile:
            c.hydro.profile(False)
    finally:
        os.environ.pop("CASTRO_AMD_SOURCES_ONE_PASS", None)
    return c


def fingerprint(c):
    out = dict(S_new=_tensor(c.S_new_b), grav_old="-", grav_new="-", phi_new="-", phi_old="-", radial="-", point_mass="-", stats="-")
    if c.grav_fab:
        out["grav_old"], out["grav_new"] = _tensor(c.grav_old), _tensor(c.grav_new)
    if c.poisson is not None:
        out["phi_new"], out["phi_old"] = _tensor(c.phi_grav(new=True)), _tensor(c.phi_grav(new=False))
        st = c.poisson_stats()
        out["stats"] = _digest(json.dumps([(k, st[k]["cycles"], [float(x).hex() for x in st[k]["history"]])
                                           for k in ("first", "old", "new")]).encode())
        out["cycles"] = "/".join(str(st[k]["cycles"]) for k in ("first", "old", "new"))
    elif c.monopole:
        out["radial"] = _digest(*[a.tobytes() for a in c.radial_gravity()])
    if c.point_mass is not None:
        out["point_mass"] = _digest(struct.pack("<d", c.point_mass))
    return out


def launches(name, numerics):
    """kernel launches of the library in the STEPS steps of configuration `name`, in a run of its own"""
    rep = {k: v[1] for k, v in run(name, "device", numerics, profile=True).hydro.profile_report().items() if v[1]}
    return sum(rep.values()), _digest(json.dumps(sorted(rep.items())).encode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=("oracle", "device"), default="oracle")
    ap.add_argument("--numerics", choices=("exact", "contract"), default="exact")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--only", nargs="*", default=sorted(CONFIGS))
    a = ap.parse_args()
    if a.backend == "device":
        import torch
        if not torch.cuda.is_available():
            sys.exit("tools/gravity_fingerprint.py --backend device needs a GPU; there is none")
    for name in a.only:
        fp = fingerprint(run(name, a.backend, a.numerics))
        if a.launches and a.backend == "device":
            fp["launches"], fp["kernels"] = launches(name, a.numerics)
        print("%s %s %s  " % (name, a.backend, a.numerics if a.backend == "device" else "-")
              + " ".join("%s=%s" % kv for kv in fp.items()), flush=True)


if __name__ == "__main__":
    main()

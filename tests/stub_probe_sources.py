"""The cases of tests/golden/stub_probe/source_vectors.npz -- inputs and outputs of the reference's own Castro::apply_sponge /
construct_new_sponge_source, construct_old/new_gravity_source and Castro::pointmass_update, compiled unmodified against stand-in
headers (tools/stub_probe/probe_sources.cpp, make_vectors.py) -- as the CPU and the GPU replay
(tests/test_stub_probe_sources.py, tests/test_stub_probe_sources_gpu.py) read them.  Only the fixture is read."""
import os
import re
import types

import numpy as np

from castro_amd import _lib

VEC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stub_probe", "source_vectors.npz")
_V = {}


def vectors():
    if not _V:
        with np.load(VEC) as f:
            _V.update({k: f[k] for k in f.files})
    return _V


def case_ids(family):
    pat = re.compile(r"in:%s(\d+)\.(box|boxes)$" % family)
    return sorted(int(m.group(1)) for m in map(pat.match, vectors()) if m)


def _get(P, name, kind="in"):
    return vectors()["%s:%s%s" % (kind, P, name)]


def geom_of(P):
    """a castro_amd_geom with the case's dx and problo as recorded (not re-derived from prob_hi and a zone count)"""
    g = _lib.make_geom((64, 64, 64))
    for d in range(3):
        g.dx[d], g.problo[d] = float(_get(P, "dx")[d]), float(_get(P, "problo")[d])
        g.probhi[d] = g.problo[d] + 64 * g.dx[d]
    return g


def _box(a):
    return tuple(int(x) for x in a[:3]), tuple(int(x) for x in a[3:6])


def same(a, b):
    """the same values, NaN where NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def differing(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


# ---- sponge ----------------------------------------------------------------------------------------------------------------------
def sponge_case(c):
    P = "sponge%d." % c
    lo, hi = _box(_get(P, "box"))
    s = lambda k: float(_get(P, k)[0])
    timescale = s("timescale")
    sp = _lib.make_sponge(1.0, lower_radius=s("lower_radius"), upper_radius=s("upper_radius"), lower_density=s("lower_density"),
                          upper_density=s("upper_density"), lower_pressure=s("lower_pressure"), upper_pressure=s("upper_pressure"),
                          lower_factor=s("lower_factor"), upper_factor=s("upper_factor"),
                          target_velocity=tuple(float(x) for x in _get(P, "target_velocity")),
                          center=tuple(float(x) for x in _get(P, "center")), implicit=int(s("implicit")))
    sp.timescale = timescale                   # make_sponge refuses what Castro.cpp:475 refuses; apply_sponge itself takes it (alpha = 0)
    ramps = [n for n in ("radius", "density", "pressure") if s("upper_" + n) > 0.0]
    return types.SimpleNamespace(P=P, lo=lo, hi=hi, box=(lo, hi), U=_get(P, "U"), dt=s("dt"), sponge=sp, geom=geom_of(P),
                                 eos_gamma=s("eos_gamma"), timescale=timescale, implicit=int(s("implicit")), ramps=ramps,
                                 step=s("lower_density") == s("upper_density") and s("upper_density") > 0.0,
                                 want=_get(P, "src", "out"))


# ---- gravity sources -------------------------------------------------------------------------------------------------------------
def gravity_case(c):
    P = "grav%d." % c
    lo, hi = _box(_get(P, "box"))
    gbox = (tuple(x - 1 for x in lo), tuple(x + 1 for x in hi))
    fb, M = [], []
    for d in range(3):
        fhi = list(hi)
        fhi[d] += 1
        fb.append((lo, tuple(fhi)))
        M.append(_get(P, "mflux%d" % d)[None])                       # (1, nz, ny, nx) of the face box
    gold = _get(P, "gold")
    const = bool(_get(P, "const")[0])
    return types.SimpleNamespace(P=P, lo=lo, hi=hi, box=(lo, hi), gbox=gbox, uold=_get(P, "uold"), unew=_get(P, "unew"), gold=gold,
                                 gnew=_get(P, "gnew"), M=M, fb=fb, gtype=int(_get(P, "grav_source_type")[0]), dt=float(_get(P, "dt")[0]),
                                 const=const, vec=tuple(float(gold[n, 0, 0, 0]) for n in range(3)) if const else None,
                                 geom=geom_of(P), want_old=_get(P, "old", "out"), want_new=_get(P, "new", "out"))


# ---- point mass ------------------------------------------------------------------------------------------------------------------
def pointmass_case(c):
    P = "pm%d." % c
    B = _get(P, "boxes")
    boxes = [_box(B[6 * b:6 * b + 6]) for b in range(B.size // 6)]
    return types.SimpleNamespace(P=P, boxes=boxes, sold=[_get(P, "sold%d" % b) for b in range(len(boxes))],
                                 snew=[_get(P, "snew%d" % b) for b in range(len(boxes))], geom=geom_of(P),
                                 center=tuple(float(x) for x in _get(P, "center")), mass=float(_get(P, "mass")[0]),
                                 want_parts=_get(P, "parts", "out"), want_delta=float(_get(P, "delta", "out")[0]),
                                 want_mass=float(_get(P, "mass", "out")[0]),
                                 want_snew=[_get(P, "snew%d" % b, "out") for b in range(len(boxes))])

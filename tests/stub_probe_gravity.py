"""The cases of tests/golden/stub_probe/gravity_vectors.npz -- inputs and outputs of the reference's own Gravity::install_level,
compute_radial_mass, make_radial_gravity, interpolate_monopole_grav, add_pointmass_to_gravity, init_multipole_grav and
fill_multipole_BCs, compiled unmodified against stand-in headers (tools/stub_probe/probe_gravity.cpp, make_gravity_vectors.py) --
as the CPU and the GPU replay (tests/test_stub_probe_gravity.py, tests/test_stub_probe_gravity_gpu.py) read them.  Only the
fixture is read."""
import os
import re
import types

import numpy as np

from castro_amd import _lib

VEC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stub_probe", "gravity_vectors.npz")
_V = {}


def vectors():
    if not _V:
        with np.load(VEC) as f:
            _V.update({k: f[k] for k in f.files})
    return _V


def case_ids(family):
    pat = re.compile(r"in:%s(\d+)\.nlev$" % family)
    return sorted(int(m.group(1)) for m in map(pat.match, vectors()) if m)


def _get(P, name, kind="in"):
    return vectors()["%s:%s%s" % (kind, P, name)]


def _has(P, name, kind="in"):
    return "%s:%s%s" % (kind, P, name) in vectors()


def same(a, b):
    """the same bits (so -0.0 is not 0.0), NaN where NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def boxes_of(P, l):
    a = [int(x) for x in _get(P, "boxes%d" % l)]
    return [(tuple(a[i:i + 3]), tuple(a[i + 3:i + 6])) for i in range(0, len(a), 6)]


def grow(b, ng):
    return tuple(x - ng for x in b[0]), tuple(x + ng for x in b[1])


def geom_of(P, l=0):
    """a castro_amd_geom of level l with dx, problo and probhi as recorded (dx halved per level: exact)"""
    flat = _has(P, "flat")
    r = 1 if flat else 2 ** l
    dom = [int(x) for x in _get(P, "domain")]
    n = tuple((dom[3 + d] - dom[d] + 1) * r for d in range(3))
    g = _lib.make_geom(n, domlo=tuple(dom[d] * r for d in range(3)))
    for d in range(3):
        g.dx[d], g.problo[d], g.probhi[d] = float(_get(P, "dx")[d]) / r, float(_get(P, "problo")[d]), float(_get(P, "probhi")[d])
    return g


def common(P):
    nlev = int(_get(P, "nlev")[0])
    return types.SimpleNamespace(P=P, nlev=nlev, flat=_has(P, "flat"), drdxfac=int(_get(P, "drdxfac")[0]),
                                 center=tuple(float(x) for x in _get(P, "center")), dx=tuple(float(x) for x in _get(P, "dx")),
                                 problo=tuple(float(x) for x in _get(P, "problo")), boxes=[boxes_of(P, l) for l in range(nlev)],
                                 numpts=[int(_get(P, "numpts%d" % l)[0]) for l in range(nlev)],
                                 n_cell=[tuple(geom_of(P, l).domhi[d] - geom_of(P, l).domlo[d] + 1 for d in range(3)) for l in range(nlev)])


def mono_of(c, l, n1d):
    return _lib.make_monopole(c.n_cell[l], geom_of(c.P, l), c.center, c.drdxfac, n1d=int(n1d))


def radial_mass_case(i):
    P = "rm%d." % i
    c = common(P)
    c.level, c.n1d = int(_get(P, "level")[0]), int(_get(P, "n1d")[0])
    c.geom = geom_of(P, c.level)
    c.mono = mono_of(c, c.level, c.n1d)
    c.bx = c.boxes[c.level]
    c.rho = [_get(P, "rho%d_%d" % (c.level, b)) for b in range(len(c.bx))]
    c.want_mass, c.want_vol = _get(P, "mass", "out"), _get(P, "vol", "out")
    return c


def time_branch(time, t_old, t_new):
    """which state make_radial_gravity bins (Gravity.cpp:2964-3006): ("new" | "old" | "mix", omalpha, alpha)"""
    eps = (t_new - t_old) * 1.e-6
    if eps == 0.0:
        return "same", 0.0, 1.0
    if abs(time - t_old) < eps:
        return "old", 1.0, 0.0
    if abs(time - t_new) < eps:
        return "new", 0.0, 1.0
    assert t_old < time < t_new
    alpha = (time - t_old) / (t_new - t_old)
    return "mix", 1.0 - alpha, alpha


def radial_gravity_case(i):
    P = "rg%d." % i
    c = common(P)
    c.level, c.time = int(_get(P, "level")[0]), float(_get(P, "time")[0])
    c.times = [(float(_get(P, "t_old%d" % l)[0]), float(_get(P, "t_new%d" % l)[0])) for l in range(c.nlev)]
    c.rho_old = [[_get(P, "rho_old%d_%d" % (l, b)) for b in range(len(c.boxes[l]))] for l in range(c.nlev)]
    c.rho_new = [[_get(P, "rho_new%d_%d" % (l, b)) for b in range(len(c.boxes[l]))] for l in range(c.nlev)]
    c.mask = [[_get(P, "mask%d_%d" % (l, b)) if _has(P, "mask%d_0" % l) else None for b in range(len(c.boxes[l]))] for l in range(c.nlev)]
    c.want_n1d = [int(x) for x in _get(P, "n1d", "out")]
    c.want_maxrad = float(_get(P, "maxrad", "out")[0])
    c.want_mass = [_get(P, "mass%d" % l, "out") for l in range(c.level + 1)]
    c.want_vol = [_get(P, "vol%d" % l, "out") for l in range(c.level + 1)]
    c.want_grav = _get(P, "grav", "out")
    c.geoms = [geom_of(P, l) for l in range(c.nlev)]
    c.monos = [mono_of(c, l, c.want_n1d[l]) for l in range(c.level + 1)]
    return c


def interpolate_case(i):
    P = "ig%d." % i
    c = common(P)
    c.level, c.ng, c.fill, c.rg = int(_get(P, "level")[0]), int(_get(P, "ng")[0]), float(_get(P, "fill")[0]), _get(P, "rg")
    c.geom = geom_of(P, c.level)
    c.mono = mono_of(c, c.level, c.rg.size)
    c.gbox = [grow(b, c.ng) for b in c.boxes[c.level]]
    c.want = [_get(P, "grav%d" % b, "out") for b in range(len(c.gbox))]
    return c


def pointmass_case(i):
    P = "pg%d." % i
    c = common(P)
    c.mass, c.ng_grav, c.ng_phi = float(_get(P, "mass")[0]), int(_get(P, "ng_grav")[0]), int(_get(P, "ng_phi")[0])
    c.geom = geom_of(P, 0)
    c.gbox, c.pbox = [grow(b, c.ng_grav) for b in c.boxes[0]], [grow(b, c.ng_phi) for b in c.boxes[0]]
    c.grav = [np.stack([_get(P, "grav%d_%d" % (n, b)) for n in range(3)]) for b in range(len(c.gbox))]
    c.phi = [_get(P, "phi%d" % b) for b in range(len(c.gbox))]
    c.want_grav = [_get(P, "grav%d" % b, "out") for b in range(len(c.gbox))]
    c.want_phi = [_get(P, "phi%d" % b, "out") for b in range(len(c.gbox))]
    return c


def multipole_case(i):
    P = "mp%d." % i
    c = common(P)
    c.lnum = int(_get(P, "lnum")[0])
    c.geoms = [geom_of(P, l) for l in range(c.nlev)]
    c.rho = [[_get(P, "rho%d_%d" % (l, b)) for b in range(len(c.boxes[l]))] for l in range(c.nlev)]
    c.mask = [[_get(P, "mask%d_%d" % (l, b)) if _has(P, "mask%d_0" % l) else None for b in range(len(c.boxes[l]))] for l in range(c.nlev)]
    c.phi, c.pbox = _get(P, "phi0"), grow(c.boxes[0][0], 1)
    for k in ("rmax", "volumeFactor", "parity_q0", "parity_qC_qS", "symmetric", "factArray", "npts", "qL0", "qLC", "qLS", "vol"):
        setattr(c, "want_" + k, _get(P, k, "out"))
    c.want_phi = _get(P, "phi0", "out")
    return c

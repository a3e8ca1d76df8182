"""tests/golden/stub_probe/bc_vectors.npz for the tests that replay it: outputs of the reference's own ambient_fill and hse_fill
(Source/problems/ambient_fill.cpp, hse_fill.cpp, compiled unmodified against stand-in headers by tools/stub_probe/probe_bc.cpp;
STUB-COMPILED, NOT oracle/_ref) on FABs whose zones outside the domain hold the generic fill.  Only the fixture is read.

case(c) gives the arguments of castro_amd_ext_bc_fill_fab as the ctypes structures of castro_amd._lib -- tests/ext_bc_ref.py reads
the same attributes -- with the input state and the recorded output."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stub_probe", "bc_vectors.npz")
_V = None


def vectors():
    global _V
    if _V is None:
        with np.load(PATH) as z:
            _V = {k: z[k] for k in z.files}
    return _V


def ncases():
    return len([k for k in vectors() if k.startswith("out:")])


def case(c):
    """(box, geom, params, ext, U_in, U_out, silent) of case c"""
    from castro_amd import _lib
    V, P = vectors(), "in:bc%d." % c
    b = [int(x) for x in V[P + "box"]]
    box = (tuple(b[:3]), tuple(b[3:]))
    domlo, domhi = [int(x) for x in V[P + "domlo"]], [int(x) for x in V[P + "domhi"]]
    dx = V[P + "dx"]
    geom = _lib.Geom()
    for d in range(3):
        geom.dx[d], geom.problo[d], geom.probhi[d] = dx[d], 0.0, dx[d] * (domhi[d] + 1)
        geom.domlo[d], geom.domhi[d] = domlo[d], domhi[d]
        geom.lo_bc[d], geom.hi_bc[d] = int(V[P + "lo_bc"][d]), int(V[P + "hi_bc"][d])
    geom.coord = 0
    small = {k: float(V[P + k][0]) for k in ("small_dens", "small_temp", "small_ener")}
    params = _lib.default_params(**small)
    assert params.eos_gamma == float(V[P + "eos_gamma"][0]) and params.abar == 1.0, "the gamma-law gas of the recording (stub/eos.H)"
    t, f = [int(x) for x in V[P + "types"]], [int(x) for x in V[P + "flags"]]
    ext = _lib.ExtBc()
    for d in range(3):
        ext.lo_type[d], ext.hi_type[d] = t[2 * d], t[2 * d + 1]
    (ext.hse_zero_vels, ext.hse_interp_temp, ext.hse_reflect_vels, ext.fill_ambient_bc, ext.ambient_fill_dir,
     ext.ambient_outflow_vel) = f
    ext.const_grav = float(V[P + "const_grav"][0])
    # the ambient state by the driver's rule; the recording holds the one the probe was given
    amb = _lib.ambient_state(params, *(float(V[P + k][0]) for k in ("ambient_density", "ambient_temp", "ambient_energy")))
    assert np.array_equal(np.array(amb), V[P + "ambient"])
    for n in range(8):
        ext.ambient_state[n] = amb[n]
    return box, geom, params, ext, V[P + "U"], V["out:bc%d.U" % c], bool(V[P + "silent"][0])


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))

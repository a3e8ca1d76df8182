"""numpy restatement of the central point mass (castro.use_point_mass): Gravity::add_pointmass_to_gravity
(Source/gravity/Gravity.cpp:2903-2948, without the phi part) and Castro::pointmass_update (Source/gravity/Castro_pointmass.cpp), in
the reference's operation order -- the CPU reference of castro_amd/csrc/pointmass_kernels.hip.  Tests only.

PointMassOracleBackend carries the three backend methods the drivers call, so Castro and CastroAmr run with a point mass on the
CPU (the separate-call path of the source stages)."""
import math

import numpy as np

from tests.monopole_amr_ref import MonopoleAmrOracleBackend
from tests.monopole_ref import _sl
from tests.sponge_ref import SpongeOracleBackend

URHO, NUM_STATE = 0, 8


def pointmass_term(box, geom, center, Gconst, M):
    """the three components (3, nz, ny, nx) the reference adds to grav on the zones of `box` = (lo, hi)"""
    lo, hi = box
    r = [geom.problo[d] + (np.arange(lo[d], hi[d] + 1).astype(np.float64) + 0.5) * geom.dx[d] - center[d] for d in range(3)]
    x, y, z = r[0][None, None, :], r[1][None, :, None], r[2][:, None, None]
    with np.errstate(all="ignore"):
        rsq = x * x + y * y + z * z
        radial_force = -Gconst * M / rsq
        rinv = 1.e0 / np.sqrt(rsq)
        return np.stack([radial_force * (np.broadcast_to(c, rsq.shape) * rinv) for c in (x, y, z)])


def add_pointmass(grav, box, geom, center, Gconst, M):
    """grav (3, nz, ny, nx) on `box`, in place: grav(n) += radial_force * (x_n * rinv) over the whole box"""
    grav += pointmass_term(box, geom, center, Gconst, M)


def cube(center, geom):
    """(lo, hi) of the zones icen - 2 .. icen + 1, icen = floor((center - problo) / dx + 1e-8) (Castro_pointmass.cpp:38-65)"""
    icen = [int(math.floor((center[d] - geom.problo[d]) / geom.dx[d] + 1.e-8)) for d in range(3)]
    return tuple(i - 2 for i in icen), tuple(i + 1 for i in icen)


def clip(cb, lo, hi):
    """the cube clipped to the box [lo, hi], or None where the box misses it"""
    clo = tuple(max(cb[0][d], lo[d]) for d in range(3))
    chi = tuple(min(cb[1][d], hi[d]) for d in range(3))
    return None if any(chi[d] < clo[d] for d in range(3)) else (clo, chi)


def delta_terms(boxes, geom, center):
    """vol * (rho_new - rho_old) of every cube zone of every box, one flat array.  boxes: [(lo, hi, S_old, obox, S_new, nbox)]"""
    vol = geom.dx[0] * geom.dx[1] * geom.dx[2]
    cb = cube(center, geom)
    out = []
    for lo, hi, So, obox, Sn, nbox in boxes:
        c = clip(cb, lo, hi)
        if c is not None:
            out.append((vol * (np.asarray(Sn)[(URHO,) + _sl(nbox, *c)] - np.asarray(So)[(URHO,) + _sl(obox, *c)])).ravel())
    return np.concatenate(out) if out else np.zeros(0)


def delta_parts(boxes, geom, center):
    """the sum of every box on its own, one accumulator over the box's cube zones in the order of the reference's loop nest (k
    outermost, i innermost; Castro_pointmass.cpp:35-79) -- a numpy sum adds in another order.  Within ONE box this is the
    reference's order; a box that misses the cube gives 0"""
    parts = []
    for b in boxes:
        s = 0.0
        for t in delta_terms([b], geom, center):
            s += float(t)
        parts.append(s)
    return parts


def delta(boxes, geom, center):
    """mass_change_at_center of this rank's boxes: the parts of delta_parts added in box order.  For one box that is the
    reference's order.  For several it is ONE of the orders the reference may take, not THE order: AMReX on one rank carries a
    single accumulator across the MFIter loop (another association), threads, ranks and a GPU reduction others again.  Any
    order is within n 2^-52 sum |terms| of any other; bit equality across several boxes can be asked only where the sum is
    exact (the multi-box cases of tests/golden/stub_probe/source_vectors.npz)"""
    s = 0.0
    for p in delta_parts(boxes, geom, center):
        s += p
    return s


def apply(boxes, geom, center, d, M):
    """the second half of pointmass_update: returns the new point mass; S_new of the boxes is changed in place"""
    if not d > 0.0:
        return M
    cb = cube(center, geom)
    for lo, hi, So, obox, Sn, nbox in boxes:
        c = clip(cb, lo, hi)
        if c is not None:
            np.asarray(Sn)[(slice(None),) + _sl(nbox, *c)] = np.asarray(So)[(slice(None),) + _sl(obox, *c)]
    return M + d


class PointMassOracleBackend(MonopoleAmrOracleBackend, SpongeOracleBackend):
    """the monopole / sponge CPU backends + the point-mass methods, in numpy.  calls: what the drivers asked for, in order"""

    def __init__(self, nthreads=1, ulps=0):
        super().__init__(nthreads, ulps)
        self.calls = []

    @staticmethod
    def make_grav_fabs(specs):
        return list(specs)

    @staticmethod
    def make_pointmass_boxes(specs):
        return list(specs), len(specs)

    def add_pointmass_mf(self, fabs, pm, geom, mass, stream=None):
        for g, box in fabs:
            self.calls.append(("add", box, g))
            add_pointmass(g.numpy(), box, geom, list(pm.center), pm.Gconst, float(mass[0]))

    @staticmethod
    def _boxes(boxes):
        return [(lo, hi, So.numpy(), obox, Sn.numpy(), nbox) for lo, hi, (So, obox), (Sn, nbox) in boxes[0]]

    def pointmass_delta_mf(self, boxes, pm, geom, delta_out, stream=None):
        d = delta(self._boxes(boxes), geom, list(pm.center))
        self.calls.append(("delta", [b[:2] for b in boxes[0]], d))
        delta_out[0] = d

    def pointmass_apply_mf(self, boxes, pm, geom, delta_in, mass, stream=None):
        mass[0] = apply(self._boxes(boxes), geom, list(pm.center), float(delta_in[0]), float(mass[0]))


# ---- the driver cases shared by the CPU and the GPU tests ------------------------------------------------------------------------
PM_N, PM_G, PM_M = (16, 16, 16), 1.0, 0.02


def radial_flow_state(params, n=PM_N, v0=-1.5, width=0.12, T0=1.e-8):
    """rho = 1, uniform temperature, a radial velocity v0 (r / width) exp(1/2 - r^2 / (2 width^2)) about the middle of the unit
    domain -- |v| peaks at r = width with |v0|; v0 < 0: inflow towards the centre, v0 > 0: outflow -- on n zones, gamma-law
    consistent (NUM_STATE, nz, ny, nx)"""
    from castro_amd import _lib
    ax = [(np.arange(n[d]) + 0.5) / n[d] - 0.5 for d in range(3)]
    X, Y, Z = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
    r = np.sqrt(X * X + Y * Y + Z * Z)
    f = v0 * np.exp(0.5 - r * r / (2.0 * width * width)) / width
    U = np.zeros((NUM_STATE,) + r.shape)
    U[0] = 1.0
    for k, c in enumerate((X, Y, Z)):
        U[1 + k] = f * np.broadcast_to(c, r.shape)
    U[5] = _lib.gamma_law_cv(params) * T0
    U[4] = U[5] + 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2)
    U[6], U[7] = T0, 1.0
    return U


def pointmass_run(hydro, params, state, steps=2, **kw):
    """(driver, [dt of every step]) of Castro(PM_N, do_grav, use_point_mass) from `state` on `hydro`"""
    import castro_amd
    kw.setdefault("point_mass", PM_M)
    c = castro_amd.Castro(PM_N, params=params, hydro=hydro, do_grav=True, use_point_mass=True, Gconst=PM_G, **kw)
    c.set_state(state)
    return c, [c.step() for _ in range(steps)]

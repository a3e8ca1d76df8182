"""numpy restatement of Poisson gravity on a refined level of SEVERAL boxes (tests only), written from the comments of
castro_amd_poisson_boxes_* in include/castro_hydro_amd.h, operation by operation: the level is ONE array over the bounding box BB
of its boxes with a byte of flags per zone, the passes are those of tests/poisson_ref.py with "beyond a domain face" replaced
by "the flag of this face is set", and the value ON such a face comes from a face array (level 0) or is 0.0 (coarser levels).
Also the coarse-fine boundary values of such a level and a CPU backend that adds the operations to
tests/poisson_amr_ref.PoissonAmrOracleBackend.  The product never imports this file.

Arrays are (nz, ny, nx).  phi-like arrays hold BB grown by one zone; the face array X is (3, nz + 1, ny + 1, nx + 1) over
[BB.lo, BB.hi + 1]: X[d] at the zone (i, j, k) is the value on the low d-face of that zone."""
import numpy as np

from tests import grid_caps as GC
from tests import monopole_ref as MR
from tests import poisson_amr_ref as A
from tests import poisson_ref as R

COVERED = 1
MAX_BOTTOM = 4096


def face_bit(d, side):
    return 2 << (2 * d + side)


# ---- the five layouts of the tests: boxes of a 32^3 level-1 index space over a 16^3 level 0, dx = 1 / 32 ----------------------------
def _cube(lo, n=8):
    return (tuple(lo), tuple(x + n - 1 for x in lo))


LAYOUTS = {
    "tile2": [_cube((8, 8, 8)), _cube((16, 8, 8))],
    "tile4": [_cube((8, 8, 8)), _cube((16, 8, 8)), _cube((8, 16, 8)), _cube((16, 16, 8))],
    "ell": [_cube((8, 8, 8)), _cube((16, 8, 8)), _cube((8, 16, 8))],
    "edge": [_cube((8, 8, 8)), _cube((16, 16, 8))],
    "disjoint": [_cube((4, 4, 4)), _cube((20, 20, 20))],
    "unequal": [_cube((8, 8, 8)), ((16, 12, 8), (19, 19, 15))],
    # aligned to 2 only: the coarsening stops at level 1, 15 x 16 x 17 of the bounding box (78 % covered) -- a bottom solve of
    # 2176 x-pairs per colour, more than one trip of its workgroup (tests/grid_caps.py)
    "wide_bottom": GC.BOTTOM_UNION,
}
# the coarse box (grown by one) under each layout: the 16^3 level 0 of the tests, or what the layout needs
CRSE_BOX = {"wide_bottom": GC.BOTTOM_UNION_CRSE_BOX}
DX = (1.0 / 32,) * 3


def bounding_box(boxes):
    return (tuple(min(b[0][d] for b in boxes) for d in range(3)), tuple(max(b[1][d] for b in boxes) for d in range(3)))


def shape_of(box, grow=0):
    return tuple(box[1][d] - box[0][d] + 1 + 2 * grow for d in (2, 1, 0))


class Plan:
    """castro_amd_poisson_boxes_plan_create: the levels (lo, n, the coefficients of poisson_ref.Level) and the flags of each"""

    def __init__(self, dx, boxes):
        self.boxes = [(tuple(b[0]), tuple(b[1])) for b in boxes]
        self.dx = tuple(float(x) for x in dx)
        for lo, hi in self.boxes:
            if any(hi[d] < lo[d] or lo[d] < 0 or lo[d] % 2 != 0 or hi[d] % 2 != 1 for d in range(3)):
                raise ValueError("a box that is not the refinement of a coarse box: %s" % ((lo, hi),))
        for n, b in enumerate(self.boxes):
            for c in self.boxes[:n]:
                if all(b[1][d] >= c[0][d] and c[1][d] >= b[0][d] for d in range(3)):
                    raise ValueError("boxes overlap: %s and %s" % (b, c))
        self.bb = bounding_box(self.boxes)
        lo, n, h = self.bb[0], tuple(self.bb[1][d] - self.bb[0][d] + 1 for d in range(3)), self.dx
        self.lo, self.lev = [lo], [R.Level(n, h)]
        while (len(self.lev) < 32 and all(x % 2 == 0 and x // 2 >= 2 for x in n)
               and all(b[s][d] % (1 << len(self.lev)) == 0 if s == 0 else (b[s][d] + 1) % (1 << len(self.lev)) == 0
                       for b in self.boxes for s in (0, 1) for d in range(3))):
            lo, n, h = tuple(x >> 1 for x in lo), tuple(x // 2 for x in n), tuple(2.0 * x for x in h)
            self.lo.append(lo)
            self.lev.append(R.Level(n, h))
        if n[0] * n[1] * n[2] > MAX_BOTTOM:
            raise ValueError("the coarsest level %s holds more than %d zones" % (n, MAX_BOTTOM))
        self.flags = [self._flags(m) for m in range(len(self.lev))]

    def _flags(self, m):
        L, lo = self.lev[m], self.lo[m]
        cov = np.zeros(L.shape, dtype=bool)
        for blo, bhi in self.boxes:
            cov[tuple(slice((blo[d] >> m) - lo[d], (bhi[d] >> m) - lo[d] + 1) for d in (2, 1, 0))] = True
        pad = np.zeros(L.gshape, dtype=bool)
        pad[1:-1, 1:-1, 1:-1] = cov
        fl = cov.astype(np.uint8) * COVERED
        for d in range(3):
            ax = 2 - d
            for side in (0, 1):
                sl = [slice(1, -1)] * 3
                sl[ax] = slice(0, -2) if side == 0 else slice(2, None)
                fl |= (cov & ~pad[tuple(sl)]).astype(np.uint8) * face_bit(d, side)
        return fl

    def covered(self, m=0):
        return (self.flags[m] & COVERED) != 0

    @property
    def phibox(self):
        return (tuple(x - 1 for x in self.bb[0]), tuple(x + 1 for x in self.bb[1]))

    @property
    def facebox(self):
        return (self.bb[0], tuple(x + 1 for x in self.bb[1]))


def _face_values(X, d, side, shape):
    """the value on the (d, side) face of every zone, from the face array X (None: 0.0)"""
    if X is None:
        return np.zeros(shape)
    nz, ny, nx = shape
    off = [0, 0, 0]
    off[2 - d] = side
    return X[d][off[0]:off[0] + nz, off[1]:off[1] + ny, off[2]:off[2] + nx]


def _parity(L):
    nz, ny, nx = L.shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (i + j + k) & 1


def smooth(L, fl, P, B, X, colour):
    """one sweep of one colour on the one-ghost array P, in place: covered zones only"""
    nb = list(R._neighbours(P)[1:])
    cs = (L.cx, L.cx, L.cy, L.cy, L.cz, L.cz)
    dg = np.full(L.shape, L.cdiag)
    for r in range(6):
        bit = (fl & face_bit(r >> 1, r & 1)) != 0
        nb[r] = np.where(bit, 2.0 * _face_values(X, r >> 1, r & 1, L.shape), nb[r])
        dg = np.where(bit, dg + cs[r], dg)
    xm, xp, ym, yp, zm, zp = nb
    off = (L.cx * (xm + xp) + L.cy * (ym + yp)) + L.cz * (zm + zp)
    new = (off - B) / dg
    sel = (_parity(L) == colour) & ((fl & COVERED) != 0)
    P[1:-1, 1:-1, 1:-1][sel] = new[sel]


def residual(L, fl, P, B, X, out):
    """r = b - lap on the covered zones of `out`, in place; the other zones of `out` keep what they hold"""
    nbs = R._neighbours(P)
    pc, nb = nbs[0], list(nbs[1:])
    for r in range(6):
        bit = (fl & face_bit(r >> 1, r & 1)) != 0
        nb[r] = np.where(bit, 2.0 * _face_values(X, r >> 1, r & 1, L.shape) - pc, nb[r])
    xm, xp, ym, yp, zm, zp = nb
    tp = 2.0 * pc
    lap = (L.cx * ((xm + xp) - tp) + L.cy * ((ym + yp) - tp)) + L.cz * ((zm + zp) - tp)
    sel = (fl & COVERED) != 0
    out[sel] = (B - lap)[sel]
    return out


def restrict(Rf, cfl, BC, PC):
    """the coarse right-hand side BC and the zeroed correction PC (one ghost) on the covered coarse zones, in place"""
    sel = (cfl & COVERED) != 0
    BC[sel] = R.restrict(Rf)[sel]
    PC[1:-1, 1:-1, 1:-1][sel] = 0.0


def prolong(PC, PF, ffl):
    sel = (ffl & COVERED) != 0
    c = PC[1:-1, 1:-1, 1:-1]
    add = PF[1:-1, 1:-1, 1:-1] + np.repeat(np.repeat(np.repeat(c, 2, axis=0), 2, axis=1), 2, axis=2)
    PF[1:-1, 1:-1, 1:-1][sel] = add[sel]


def norm(Xa, fl):
    v = Xa[(fl & COVERED) != 0]
    return float(np.max(np.abs(v))), float(np.max(v))


def vcycle(plan, phi, rhs, res, X, l=0):
    L, fl = plan.lev[l], plan.flags[l]
    Xl = X if l == 0 else None
    if l + 1 == len(plan.lev):
        for _ in range(R.NBOTTOM):
            smooth(L, fl, phi[l], rhs[l], Xl, 0)
            smooth(L, fl, phi[l], rhs[l], Xl, 1)
        return
    for _ in range(R.NPRE):
        smooth(L, fl, phi[l], rhs[l], Xl, 0)
        smooth(L, fl, phi[l], rhs[l], Xl, 1)
    residual(L, fl, phi[l], rhs[l], Xl, res[l])
    restrict(res[l], plan.flags[l + 1], rhs[l + 1], phi[l + 1])
    vcycle(plan, phi, rhs, res, X, l + 1)
    prolong(phi[l + 1], phi[l], fl)
    for _ in range(R.NPOST):
        smooth(L, fl, phi[l], rhs[l], Xl, 0)
        smooth(L, fl, phi[l], rhs[l], Xl, 1)


def solve(plan, phi, X, rho, fourpiG, reltol=1.e-10, abstol=1.e-10, maxiter=40):
    """castro_amd_poisson_boxes_solve on the one-ghost array phi over BB (in place); rho: an array over BB whose covered zones hold
    the density.  Returns (cycles, converged, final norm, history)."""
    nl = len(plan.lev)
    fl = plan.flags[0]
    b = np.zeros(plan.lev[0].shape)
    b[plan.covered()] = (fourpiG * np.asarray(rho, dtype=np.float64))[plan.covered()]
    P = [phi] + [np.zeros(plan.lev[m].gshape) for m in range(1, nl)]
    B = [b] + [np.zeros(plan.lev[m].shape) for m in range(1, nl)]
    Rs = [np.zeros(plan.lev[m].shape) for m in range(nl)]
    bnorm, max_rhs = norm(b, fl)
    rnorm = norm(residual(plan.lev[0], fl, phi, b, X, Rs[0]), fl)[0]
    t1, t2 = reltol * bnorm, abstol * max_rhs
    tol = t1 if t1 > t2 else t2
    hist = [bnorm, max_rhs, rnorm]
    n = 0
    while not (rnorm <= tol) and n < maxiter:
        vcycle(plan, P, B, Rs, X)
        rnorm = norm(residual(plan.lev[0], fl, phi, b, X, Rs[0]), fl)[0]
        n += 1
        hist.append(rnorm)
    return n, bool(rnorm <= tol), rnorm, hist


def grad_phi(plan, phi, X, mag=None):
    """g (3, nz, ny, nx) over BB, NaN where not covered: castro_amd_grad_phi_to_grav_boxes"""
    L, fl = plan.lev[0], plan.flags[0]
    nbs = R._neighbours(phi)
    pc = nbs[0]
    g = np.full((3,) + L.shape, np.nan)
    sel = plan.covered()
    for d in range(3):
        dl, dh = pc - nbs[1 + 2 * d], nbs[2 + 2 * d] - pc
        dl = np.where((fl & face_bit(d, 0)) != 0, 2.0 * (pc - _face_values(X, d, 0, L.shape)), dl)
        dh = np.where((fl & face_bit(d, 1)) != 0, 2.0 * (_face_values(X, d, 1, L.shape) - pc), dh)
        gl, gh = dl / plan.dx[d], dh / plan.dx[d]
        g[d][sel] = (-(0.5 * (gl + gh)))[sel]
        if mag is not None:
            mag[d] = 0.5 * (np.abs(gl) + np.abs(gh))
    return g


# ---- the coarse-fine boundary values of the level ------------------------------------------------------------------------------------
def cf_faces(plan, X, crse_old, cobox, crse_new, cnbox, a, mag=False):
    """castro_amd_poisson_boxes_cf_bc on the face array X, in place: for every flagged face of a covered zone the value of
    castro_amd_poisson_cf_bc_fab for the face zone g (the uncovered neighbour) -- c = oma * old + a * new, m = 0.5 * (c_out + c_in),
    value = (m0 + s1 * (0.125 * (m1p - m1m))) + s2 * (0.125 * (m2p - m2m)).  mag: the sums of the magnitudes of the terms.
    Returns the mask of the slots written, like X."""
    bb = plan.bb
    clo = tuple((x >> 1) - 1 for x in bb[0])
    chi = tuple((x >> 1) + 1 for x in bb[1])
    O, N = A._sub(crse_old, cobox, clo, chi), A._sub(crse_new, cnbox, clo, chi)
    oma = 1.0 - a
    C = np.abs(oma * O) + np.abs(a * N) if mag else oma * O + a * N
    nz, ny, nx = plan.lev[0].shape
    k, j, i = np.meshgrid(np.arange(nz) + bb[0][2], np.arange(ny) + bb[0][1], np.arange(nx) + bb[0][0], indexing="ij")
    fl = plan.flags[0]
    wrote = np.zeros(X.shape, dtype=bool)
    for d in range(3):
        t1, t2 = (1 if d == 0 else 0), (1 if d == 2 else 2)
        for side in (0, 1):
            g = [i.copy(), j.copy(), k.copy()]
            g[d] = g[d] + (1 if side else -1)
            c_out = g[d] >> 1
            c_in = c_out - 1 if side else c_out + 1

            def mean(o1, o2):
                c = [g[0] >> 1, g[1] >> 1, g[2] >> 1]
                c[t1] = c[t1] + o1
                c[t2] = c[t2] + o2
                at = lambda cd: C[tuple((cd if e == d else c[e]) - clo[e] for e in (2, 1, 0))]
                return 0.5 * (at(c_out) + at(c_in))
            m0, m1p, m1m, m2p, m2m = mean(0, 0), mean(1, 0), mean(-1, 0), mean(0, 1), mean(0, -1)
            if mag:
                v = (m0 + 0.125 * (m1p + m1m)) + 0.125 * (m2p + m2m)
            else:
                s1, s2 = np.where(g[t1] & 1, 1.0, -1.0), np.where(g[t2] & 1, 1.0, -1.0)
                v = (m0 + s1 * (0.125 * (m1p - m1m))) + s2 * (0.125 * (m2p - m2m))
            sel = ((fl & COVERED) != 0) & ((fl & face_bit(d, side)) != 0)
            off = [0, 0, 0]
            off[2 - d] = side
            view = X[d][off[0]:off[0] + nz, off[1]:off[1] + ny, off[2]:off[2] + nx]
            view[sel] = v[sel]
            wrote[d][off[0]:off[0] + nz, off[1]:off[1] + ny, off[2]:off[2] + nx][sel] = True
    return wrote


def masked_residual64(plan, phi, X, b):
    """max |b - lap(phi)| over the covered zones with the masked operator, recomputed here in float64"""
    out = np.zeros(plan.lev[0].shape)
    residual(plan.lev[0], plan.flags[0], phi, b, X, out)
    return float(np.abs(out[plan.covered()]).max())


# ---- the backend ---------------------------------------------------------------------------------------------------------------------
class PoissonBoxesOracleBackend(A.PoissonAmrOracleBackend):
    """PoissonAmrOracleBackend + the operations of a level of several boxes, in numpy"""

    def poisson_boxes_plan_create(self, dx, boxes):
        return Plan(dx, boxes)

    def poisson_boxes_cf_bc(self, plan, faces, faces_box, crse_old, crse_old_box, crse_new, crse_new_box, a, stream=None):
        assert faces_box == plan.facebox
        cf_faces(plan, faces.numpy(), crse_old.numpy()[0], crse_old_box, crse_new.numpy()[0], crse_new_box, a)

    def poisson_boxes_solve(self, plan, phi, phi_box, faces, faces_box, rhos, rho_comp, fourpiG, reltol=1.e-10, abstol=1.e-10,
                            maxiter=40, stream=None):
        assert phi_box == plan.phibox and faces_box == plan.facebox and len(rhos) == len(plan.boxes)
        rho = np.zeros(plan.lev[0].shape)
        for (S, sbox), (lo, hi) in zip(rhos, plan.boxes):
            rho[MR._sl(plan.bb, lo, hi)] = S.numpy()[(rho_comp,) + MR._sl(sbox, lo, hi)]
        return solve(plan, phi.numpy()[0], faces.numpy(), rho, fourpiG, reltol, abstol, maxiter)

    def grad_phi_to_grav_boxes(self, plan, phi, phi_box, faces, faces_box, gravs, stream=None):
        assert phi_box == plan.phibox and len(gravs) == len(plan.boxes)
        g = grad_phi(plan, phi.numpy()[0], faces.numpy())
        for (G, gbox), (lo, hi) in zip(gravs, plan.boxes):
            G.numpy()[(slice(None),) + MR._sl(gbox, lo, hi)] = g[(slice(None),) + MR._sl(plan.bb, lo, hi)]


# ---- the dust-collapse hierarchies shared by the CPU and the GPU driver tests: poisson_ref's DUST_* case on 16^3 with the three
# boxes of the layout "ell" as level 1, with two boxes nested in them as level 2, and a tagged, clustered level 1 ---------------------
ELL_CRSE = [((4, 4, 4), (7, 7, 7)), ((8, 4, 4), (11, 7, 7)), ((4, 8, 4), (7, 11, 7))]     # the layout "ell" in coarse zones
NESTED2 = [((10, 10, 10), (13, 13, 13)), ((18, 10, 10), (21, 13, 13))]      # level-1 zones inside the boxes 8..15 and 16..23 of the ell
CASES = {"ell": dict(patches=[ELL_CRSE]), "nested": dict(patches=[ELL_CRSE, NESTED2], max_level=2)}
# a ball of radius 3.5e8: its edge lies 3.7 coarse zones from the centre, away from the domain boundary; the density-gradient
# tag marks the shell at the edge, which the clustering cuts into 37 boxes of 4 and 8 level-1 zones a side around an untagged core
CLUSTER_TAGS = [("density", "gradient", 1.e8)]
CLUSTER_PROB = dict(R.DUST_PROB, r_0=3.5e8)
CLUSTER_KW = dict(refine=CLUSTER_TAGS, cluster=True, regrid_int=1000, max_level=1, blocking_factor=4, max_grid_size=8, n_error_buf=0)


def _hierarchy(make_hydro, params, **kw):
    import castro_amd
    return castro_amd.CastroAmr(A.AMR_N, params=params, make_hydro=make_hydro, do_grav=True,
                                gravity=castro_amd.PoissonGravity(center=R.DUST_CENTER), **R.DUST_GEOM, **kw)


def dust_boxes_run(make_hydro, params, case, steps=2):
    """(hierarchy, [dt of every coarse step]) of the dust collapse on the hierarchy CASES[case]"""
    a = _hierarchy(make_hydro, params, **CASES[case])
    a.initData("dust_collapse", **R.DUST_PROB)
    return a, [a.step() for _ in range(steps)]


def clustered_run(make_hydro, params):
    """(hierarchy, dts, the box lists of level 1 before and after the regrid): one step on the clustered level, a regrid with a
    buffer of one zone around the tags -- another box list --, one more step"""
    a = _hierarchy(make_hydro, params, **CLUSTER_KW)
    a.initData("dust_collapse", **CLUSTER_PROB)
    first = [b.bx for b in a.lev[1].boxes] if len(a.lev) > 1 else []
    dts = [a.step()]
    a.n_error_buf = 1
    a.regrid(0)
    second = [b.bx for b in a.lev[1].boxes] if len(a.lev) > 1 else []
    dts.append(a.step())
    return a, dts, (first, second)


def _np(t):
    return t.cpu().numpy().copy()


def level_fields(a):
    """[([S_new of every box], phi of the level on its bounding box, covered, [grav_new of every box])] per level, numpy"""
    out = []
    for l, lev in enumerate(a.lev):
        _, phi, cov = a.phi_grav_level(l)
        out.append(([_np(b.S_new()) for b in lev.boxes], phi, cov, [_np(b.grav_new) for b in lev.boxes]))
    return out


def sensitivity(run, *args):
    """(reference fields, its other results, s per level): `run(make_hydro, *args)` on PoissonBoxesOracleBackend and the largest
    deviation per field over the boxes of a level of a second run whose moments are scaled by 1 + 2**-52 (the rule of
    poisson_ref.dust_sensitivity)"""
    ref = run(lambda: PoissonBoxesOracleBackend(), *args)
    ulp = run(lambda: PoissonBoxesOracleBackend(scale=1.0 + R.U52), *args)
    fr, fu = level_fields(ref[0]), level_fields(ulp[0])
    s = [np.max([MR.field_deviation(u, r) for u, r in zip(U[0], Rf[0])], axis=0) for U, Rf in zip(fu, fr)]
    return fr, ref, s

"""numpy restatement of Poisson gravity (tests only), written from the definitions in include/castro_hydro_amd.h and the header
comments of castro_amd/csrc/poisson_kernels.hip -- operation by operation, in that order --, and a CPU backend that adds the
Poisson methods of castro_amd.hydro.HipHydro to tests/monopole_ref.MonopoleOracleBackend.  The product never imports this file.

Multigrid.  The five passes hold additions, multiplications and divisions only: the `exact` build (no contraction) gives the
bits of this file; the `contract` build fuses multiply-adds, which moves a result by less than one rounding per fused pair --
the tests grant it 8 * 2**-52 of the sum of the magnitudes of the terms of each result (*_mag below).

Multipole moments: the tolerance of a comparison with a device (derived, not tuned).  u = 2**-52.  A moment is a sum of N terms.
  (a) Order.  Any order of N double additions is within (N - 1) * 2**-53 * A of the exact sum, A = fsum(|t_i|); the restatement
      takes the exactly rounded sum math.fsum, so the order costs N * u * A (the bound of monopole_ref.mass_bounds).
  (b) Terms.  The kernels are compiled without contraction in both builds, so everything up to the arguments of pow, atan2, sin
      and cos is the restatement's bits (+, -, *, / and sqrt are correctly rounded on both sides).  Each CALL of the four may
      differ between the device's library and numpy's by 4 u of its result -- the allowance tests/test_sponge_gpu.py grants the
      device cos.  For a term t = a * c * (rho * p) * vol * f  (a: Legendre or associated Legendre value, c: cos(m phi) or sin(m phi)
      or 1, p = pow(r, l), f: factArray):
        p:    |dp| <= 4 u |p|
        phi:  |dphi| <= 4 u |phi|, the product m * phi rounds once more: |d(m phi)| <= 5 u m |phi|; through cos / sin, whose
              derivative is at most 1, plus the call itself: |dc| <= 5 u m |phi| + 4 u   (the amplification m |phi_angle|)
        a:    the Legendre values P_l are pure arithmetic: da = 0.  The associated ones start from P_m^m, which holds one pow:
              E_m = 4 u |P_m^m|; the recurrence is linear, so the error bound follows it with magnitudes, each step re-rounding
              its three operations: E_{m+1} = |x| (2m+1) E_m + 2 u |a_{m+1}|,
              E_l = (|x| (2l-1) E_{l-1} + (l+m-1) E_{l-2}) / (l-m) + 3 u (|x (2l-1) a_{l-1}| + |(l+m-1) a_{l-2}|) / (l-m)
        the four products after the first differing factor re-round: 4 u |t|
      dt <= (E_a |c| + |a| dc) |rho p vol f| + |t| (4 u [pow] + 4 u [products])
  bound(moment) = N u A + sum_i dt_i.
The boundary potential sums the same kind of terms in the kernel's own order (l, then m and l): its bound per ghost zone is the
sum of the dt of its terms plus n_terms * u * sum |terms| for the re-rounded partial sums, times G / rmax (+ 2 u for the last two
operations)."""
import math

import numpy as np

from tests import monopole_ref as MR

U52 = 2.0 ** -52
URHO = 0


# ---- Legendre functions (Gravity_util.H), vectorised over x ------------------------------------------------------------------
def leg_step(l, st, x):
    """calcLegPolyL: st = [P_l, P_{l-1}, P_{l-2}] updated in place for order l"""
    if l == 0:
        st[0] = np.ones_like(x)
    elif l == 1:
        st[1] = st[0]
        st[0] = x.copy()
    else:
        st[2] = st[1]
        st[1] = st[0]
        st[0] = ((2 * l - 1) * x * st[1] - (l - 1) * st[2]) / l


def assoc_step(l, m, st, x, err=None, libm=False):
    """calcAssocLegPolyLM; err (a list like st): the error bound E of the module docstring, carried along.  libm: the one pow of
    P_m^m is taken from the C library (math.pow, zone by zone) instead of numpy's vectorised pow, whose last bit can differ --
    the replay of a recording made by a C++ program then has that program's bits"""
    if l == m:
        base = (1.0 - x) * (1.0 + x)
        pw = np.array([math.pow(float(v), m * 0.5) for v in base.ravel()]).reshape(base.shape) if libm else np.power(base, m * 0.5)
        a = (-1.0 if m & 1 else 1.0) * pw
        for n in range(2 * m - 1, 2, -2):
            a = a * n
        st[0] = a
        if err is not None:
            err[0] = 4.0 * U52 * np.abs(a)
    elif l == m + 1:
        st[1] = st[0]
        st[0] = x * (2 * m + 1) * st[1]
        if err is not None:
            err[1] = err[0]
            err[0] = np.abs(x) * (2 * m + 1) * err[1] + 2.0 * U52 * np.abs(st[0])
    else:
        st[2] = st[1]
        st[1] = st[0]
        st[0] = (x * (2 * l - 1) * st[1] - (l + m - 1) * st[2]) / (l - m)
        if err is not None:
            err[2] = err[1]
            err[1] = err[0]
            err[0] = ((np.abs(x) * (2 * l - 1) * err[1] + (l + m - 1) * err[2]) / (l - m)
                      + 3.0 * U52 * (np.abs(x * (2 * l - 1) * st[1]) + np.abs((l + m - 1) * st[2])) / (l - m))


def factorial(n):
    fact = 1.0
    for i in range(2, n + 1):
        fact *= float(i)
    return fact


def fact_array(l, m):
    return 2.0 * factorial(l - m) / factorial(l + m)


def qindex(lnum, kind, l, m):
    n1 = lnum + 1
    return (kind * n1 + l) * n1 + m


# ---- moments ---------------------------------------------------------------------------------------------------------------------
def zone_geometry(lo, shape, geom, mp):
    """x, y, z (divided by rmax), r, cosTheta, phiAngle of the zone centres of a box, each (nz, ny, nx)"""
    nz, ny, nx = shape
    ax = []
    for d, n in enumerate((nx, ny, nz)):
        v = (geom.problo[d] + (np.arange(lo[d], lo[d] + n, dtype=np.float64) + 0.5) * geom.dx[d] - mp.center[d]) / mp.rmax
        sh = [1, 1, 1]
        sh[2 - d] = n
        ax.append(v.reshape(sh) + np.zeros(shape))
    x, y, z = ax
    r = np.sqrt(x * x + y * y + z * z)
    with np.errstate(all="ignore"):
        cosT = z / r
    return x, y, z, r, cosT, np.arctan2(y, x)


def zone_terms(lnum, cosT, phiA, r, rho, vol):
    """multipole_add of Gravity_util.H for zones in the last radial bin (index <= n, parity factors 1, volumeFactor 1), vectorised
    over the zones: {(kind, l, m): (terms, dt)} -- kind 0 = dQL0, 1 = dQLC, 2 = dQLS; dt: the per-term allowance of the module
    docstring"""
    out = {}
    st = [None, None, None]
    for l in range(lnum + 1):
        leg_step(l, st, cosT)
        p = np.power(r, float(l))
        t = st[0] * (rho * p) * vol
        out[(0, l, 0)] = (t, np.abs(t) * (8.0 * U52))
    for m in range(1, lnum + 1):
        cm, sm = np.cos(m * phiA), np.sin(m * phiA)
        dc = 5.0 * U52 * m * np.abs(phiA) + 4.0 * U52
        st, err = [None, None, None], [None, None, None]
        for l in range(m, lnum + 1):
            assoc_step(l, m, st, cosT, err)
            rest = rho * np.power(r, float(l))
            f = fact_array(l, m)
            for kind, c in ((1, cm), (2, sm)):
                t = st[0] * c * rest * vol * f
                dt = (err[0] * np.abs(c) + np.abs(st[0]) * dc) * np.abs(rest * vol * f) + np.abs(t) * (8.0 * U52)
                out[(kind, l, m)] = (t, dt)
    return out


def moment_terms(boxes, geom, mp):
    """boxes: [(rho (nz, ny, nx) of the valid zones, lo, mask or None)].  {(kind, l, m): (terms, dt)} -- the terms of every moment
    over all unmasked zones in box order and their allowances"""
    rmax_cubed_inv = 1.0 / (mp.rmax * mp.rmax * mp.rmax)
    vol = (geom.dx[0] * geom.dx[1] * geom.dx[2]) * rmax_cubed_inv
    out = {}
    for rho, lo, mask in boxes:
        rho = np.asarray(rho, dtype=np.float64)
        keep = np.ones(rho.shape, dtype=bool) if mask is None else (np.asarray(mask) != 0)
        x, y, z, r, cosT, phiA = zone_geometry(lo, rho.shape, geom, mp)
        for key, (t, dt) in zone_terms(mp.lnum, cosT[keep], phiA[keep], r[keep], rho[keep], vol).items():
            a, b = out.setdefault(key, ([], []))
            a.append(t)
            b.append(dt)
    return {k: (np.concatenate(a), np.concatenate(b)) for k, (a, b) in out.items()}


def moments(boxes, geom, mp):
    """(q, bound): the moments in the layout of castro_amd_multipole_moments_mf (exactly rounded sums) and the tolerance of a
    comparison with a device per entry"""
    n1 = mp.lnum + 1
    q, bound = np.zeros(3 * n1 * n1), np.zeros(3 * n1 * n1)
    for (kind, l, m), (t, dt) in moment_terms(boxes, geom, mp).items():
        i = qindex(mp.lnum, kind, l, m)
        q[i] = math.fsum(t.tolist())
        bound[i] = t.size * U52 * math.fsum(np.abs(t).tolist()) + math.fsum(dt.tolist())
    return q, bound


# ---- boundary potential ----------------------------------------------------------------------------------------------------------
def phi_bc(q, geom, mp, phi, box):
    """castro_amd_multipole_phi_bc_fab on `phi` (nz, ny, nx) of `box`, in place: the zones outside the domain.  Returns
    (outside mask, allowance per zone)."""
    lnum = mp.lnum
    shape = phi.shape
    nz, ny, nx = shape
    loc, out_d = [], []
    for d, n in enumerate((nx, ny, nz)):
        idx = np.arange(box[0][d], box[0][d] + n)
        f = idx.astype(np.float64)
        v = np.where(idx > geom.domhi[d], geom.problo[d] + f * geom.dx[d] - mp.center[d],
                     np.where(idx < geom.domlo[d], geom.problo[d] + (f + 1.0) * geom.dx[d] - mp.center[d],
                              geom.problo[d] + (f + 0.5) * geom.dx[d] - mp.center[d]))
        v = v / mp.rmax
        sh = [1, 1, 1]
        sh[2 - d] = n
        loc.append(v.reshape(sh) + np.zeros(shape))
        out_d.append(((idx < geom.domlo[d]) | (idx > geom.domhi[d])).reshape(sh) | np.zeros(shape, dtype=bool))
    outside = out_d[0] | out_d[1] | out_d[2]
    x, y, z = loc
    r = np.sqrt(x * x + y * y + z * z)
    rmax_cubed = mp.rmax * mp.rmax * mp.rmax
    with np.errstate(all="ignore"):
        cosT = z / r
        phiA = np.arctan2(y, x)
        acc = np.zeros(shape)
        mag = np.zeros(shape)
        dsum = np.zeros(shape)
        nterms = 0
        st = [None, None, None]
        for l in range(lnum + 1):
            leg_step(l, st, cosT)
            r_U = np.power(r, float(-l - 1))
            T = q[qindex(lnum, 0, l, 0)] * st[0] * r_U * rmax_cubed
            acc = acc + T
            mag += np.abs(T)
            dsum += np.abs(T) * (8.0 * U52)
            nterms += 1
        for m in range(1, lnum + 1):
            st, err = [None, None, None], [None, None, None]
            dc = 5.0 * U52 * m * np.abs(phiA) + 4.0 * U52
            for l in range(m, lnum + 1):
                assoc_step(l, m, st, cosT, err)
                r_U = np.power(r, float(-l - 1))
                qc, qs = q[qindex(lnum, 1, l, m)], q[qindex(lnum, 2, l, m)]
                amp = qc * np.cos(m * phiA) + qs * np.sin(m * phiA)
                T = amp * st[0] * r_U * rmax_cubed
                acc = acc + T
                mag += np.abs(T)
                damp = (abs(qc) + abs(qs)) * dc + 3.0 * U52 * (np.abs(qc * np.cos(m * phiA)) + np.abs(qs * np.sin(m * phiA)))
                dsum += (damp * np.abs(st[0]) + np.abs(amp) * err[0]) * np.abs(r_U * rmax_cubed) + np.abs(T) * (8.0 * U52)
                nterms += 1
        val = -mp.Gconst * acc / mp.rmax
        allow = (mp.Gconst / mp.rmax) * (dsum + nterms * U52 * mag) + 2.0 * U52 * np.abs(val)
    val = np.where(r < 1.0e-12, 0.0, val)
    allow = np.where(r < 1.0e-12, 0.0, allow)
    phi[outside] = val[outside]
    return outside, allow


# ---- multigrid -------------------------------------------------------------------------------------------------------------------
class Level:
    """one level: extents n (x, y, z), cx, cy, cz, cdiag as poisson_levels forms them"""

    def __init__(self, n, h):
        self.n = tuple(int(v) for v in n)
        self.h = tuple(float(v) for v in h)
        self.cx, self.cy, self.cz = (1.0 / (v * v) for v in self.h)
        self.cdiag = 2.0 * ((self.cx + self.cy) + self.cz)

    @property
    def shape(self):
        return (self.n[2], self.n[1], self.n[0])

    @property
    def gshape(self):
        return (self.n[2] + 2, self.n[1] + 2, self.n[0] + 2)


def levels(n_cell, dx):
    out = [Level(n_cell, dx)]
    while all(v % 2 == 0 and v // 2 >= 2 for v in out[-1].n) and len(out) < 32:
        out.append(Level([v // 2 for v in out[-1].n], [2.0 * v for v in out[-1].h]))
    return out


def _neighbours(P):
    """(pc, xm, xp, ym, yp, zm, zp) of the valid zones of a one-ghost array (nz + 2, ny + 2, nx + 2), as copies"""
    c = P[1:-1, 1:-1, 1:-1]
    return (c.copy(), P[1:-1, 1:-1, :-2].copy(), P[1:-1, 1:-1, 2:].copy(), P[1:-1, :-2, 1:-1].copy(), P[1:-1, 2:, 1:-1].copy(),
            P[:-2, 1:-1, 1:-1].copy(), P[2:, 1:-1, 1:-1].copy())


def _faces(L):
    nz, ny, nx = L.shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (i == 0, i == nx - 1, j == 0, j == ny - 1, k == 0, k == nz - 1), (i + j + k) & 1


def smooth(L, P, B, colour, mag=None):
    """k_mg_smooth: one sweep of one colour on the one-ghost array P, in place.  mag (an array like B, or None): the sum of the
    magnitudes of the terms of every updated value, (cx (|xm| + |xp|) + ... + |b|) / dg"""
    pc, xm, xp, ym, yp, zm, zp = _neighbours(P)
    (xl, xh, yl, yh, zl, zh), par = _faces(L)
    dg = np.full(L.shape, L.cdiag)
    xm = np.where(xl, 2.0 * xm, xm); dg = np.where(xl, dg + L.cx, dg)
    xp = np.where(xh, 2.0 * xp, xp); dg = np.where(xh, dg + L.cx, dg)
    ym = np.where(yl, 2.0 * ym, ym); dg = np.where(yl, dg + L.cy, dg)
    yp = np.where(yh, 2.0 * yp, yp); dg = np.where(yh, dg + L.cy, dg)
    zm = np.where(zl, 2.0 * zm, zm); dg = np.where(zl, dg + L.cz, dg)
    zp = np.where(zh, 2.0 * zp, zp); dg = np.where(zh, dg + L.cz, dg)
    off = (L.cx * (xm + xp) + L.cy * (ym + yp)) + L.cz * (zm + zp)
    new = (off - B) / dg
    sel = par == colour
    P[1:-1, 1:-1, 1:-1][sel] = new[sel]
    if mag is not None:
        m = (L.cx * (np.abs(xm) + np.abs(xp)) + L.cy * (np.abs(ym) + np.abs(yp)) + L.cz * (np.abs(zm) + np.abs(zp)) + np.abs(B)) / dg
        mag[sel] = m[sel]


def residual(L, P, B, mag=None):
    """k_mg_residual"""
    pc, xm, xp, ym, yp, zm, zp = _neighbours(P)
    (xl, xh, yl, yh, zl, zh), _ = _faces(L)
    xm = np.where(xl, 2.0 * xm - pc, xm)
    xp = np.where(xh, 2.0 * xp - pc, xp)
    ym = np.where(yl, 2.0 * ym - pc, ym)
    yp = np.where(yh, 2.0 * yp - pc, yp)
    zm = np.where(zl, 2.0 * zm - pc, zm)
    zp = np.where(zh, 2.0 * zp - pc, zp)
    tp = 2.0 * pc
    lap = (L.cx * ((xm + xp) - tp) + L.cy * ((ym + yp) - tp)) + L.cz * ((zm + zp) - tp)
    if mag is not None:
        # the ghost 2 g - p is itself a sum: its terms |2 g| and |p| both count
        a = [np.abs(v) for v in (xm, xp, ym, yp, zm, zp)]
        g = _neighbours(P)
        for n, f in enumerate((xl, xh, yl, yh, zl, zh)):
            a[n] = np.where(f, 2.0 * np.abs(g[n + 1]) + np.abs(pc), a[n])
        mag[...] = (L.cx * (a[0] + a[1] + np.abs(tp)) + L.cy * (a[2] + a[3] + np.abs(tp)) + L.cz * (a[4] + a[5] + np.abs(tp))
                    + np.abs(B))
    return B - lap


def restrict(R, mag=None):
    """k_mg_restrict: the coarse right-hand side of the fine residual R (nz, ny, nx)"""
    c = [R[c_::2, b::2, a::2] for c_ in (0, 1) for b in (0, 1) for a in (0, 1)]      # r000, r100, r010, r110, r001, ...
    s = c[0] + c[1]
    for t in c[2:]:
        s = s + t
    if mag is not None:
        mag[...] = sum(np.abs(t) for t in c) * 0.125
    return s * 0.125


def prolong(PC, PF):
    """k_mg_prolong: the one-ghost fine array PF += the valid zones of the one-ghost coarse array PC, piecewise constant"""
    c = PC[1:-1, 1:-1, 1:-1]
    PF[1:-1, 1:-1, 1:-1] = PF[1:-1, 1:-1, 1:-1] + np.repeat(np.repeat(np.repeat(c, 2, axis=0), 2, axis=1), 2, axis=2)


def norm(X):
    """k_mg_norm_*: (max |x|, max x); a NaN anywhere gives NaN"""
    return float(np.max(np.abs(X))), float(np.max(X))


NPRE, NPOST, NBOTTOM = 2, 2, 32


def vcycle(lev, phi, rhs, l=0):
    L = lev[l]
    if l + 1 == len(lev):
        for _ in range(NBOTTOM):
            smooth(L, phi[l], rhs[l], 0)
            smooth(L, phi[l], rhs[l], 1)
        return
    for _ in range(NPRE):
        smooth(L, phi[l], rhs[l], 0)
        smooth(L, phi[l], rhs[l], 1)
    rhs[l + 1] = restrict(residual(L, phi[l], rhs[l]))
    phi[l + 1] = np.zeros(lev[l + 1].gshape)
    vcycle(lev, phi, rhs, l + 1)
    prolong(phi[l + 1], phi[l])
    for _ in range(NPOST):
        smooth(L, phi[l], rhs[l], 0)
        smooth(L, phi[l], rhs[l], 1)


def solve(n_cell, dx, phi, rho, fourpiG, reltol=1.e-10, abstol=1.e-10, maxiter=40):
    """castro_amd_poisson_solve on the one-ghost array phi (in place).  Returns (cycles, converged, final norm, history)."""
    lev = levels(n_cell, dx)
    b = fourpiG * np.asarray(rho, dtype=np.float64)
    bnorm, max_rhs = norm(b)
    P, B = [phi] + [None] * (len(lev) - 1), [b] + [None] * (len(lev) - 1)
    rnorm = norm(residual(lev[0], phi, b))[0]
    t1, t2 = reltol * bnorm, abstol * max_rhs
    tol = t1 if t1 > t2 else t2
    hist = [bnorm, max_rhs, rnorm]
    n = 0
    while not (rnorm <= tol) and n < maxiter:
        vcycle(lev, P, B)
        rnorm = norm(residual(lev[0], phi, b))[0]
        n += 1
        hist.append(rnorm)
    return n, bool(rnorm <= tol), rnorm, hist


def stopping_tolerance(b, reltol=1.e-10, abstol=1.e-10):
    bnorm, max_rhs = norm(b)
    return max(reltol * bnorm, abstol * max_rhs)


def dense_operator(L):
    """(A, index): the operator of residual() as a dense matrix over the zones (k, j, i) in C order -- lap(phi) = A phi + (the
    part of the ghost values), so that A phi = b - bc"""
    nz, ny, nx = L.shape
    N = nx * ny * nz
    A = np.zeros((N, N))
    idx = np.arange(N).reshape(L.shape)
    for axis, cf, n in ((2, L.cx, nx), (1, L.cy, ny), (0, L.cz, nz)):
        for side in (-1, 1):
            for k in range(nz):
                for j in range(ny):
                    for i in range(nx):
                        p = [k, j, i]
                        row = idx[k, j, i]
                        A[row, row] -= cf
                        p[axis] += side
                        if 0 <= p[axis] < n:
                            A[row, idx[tuple(p)]] += cf
                        else:
                            A[row, row] -= cf           # the ghost 2 g - p: - p here, 2 g on the right-hand side
    return A


def boundary_rhs(L, phi):
    """the part of lap(phi) that the ghost values g contribute: sum over the boundary faces of c * 2 g, per zone"""
    out = np.zeros(L.shape)
    out[:, :, 0] += L.cx * 2.0 * phi[1:-1, 1:-1, 0]
    out[:, :, -1] += L.cx * 2.0 * phi[1:-1, 1:-1, -1]
    out[:, 0, :] += L.cy * 2.0 * phi[1:-1, 0, 1:-1]
    out[:, -1, :] += L.cy * 2.0 * phi[1:-1, -1, 1:-1]
    out[0, :, :] += L.cz * 2.0 * phi[0, 1:-1, 1:-1]
    out[-1, :, :] += L.cz * 2.0 * phi[-1, 1:-1, 1:-1]
    return out


def dense_check(L, phi, b):
    """The dense check of a solve on level L: (deviation, bound) with
    bound = ||A^-1||_inf (||r||_inf + ||r_dense||_inf + gamma), gamma = 16 * 2**-52 * || |A| |phi| ||_inf, both residuals
    recomputed in float64 from A, every term computed."""
    A = dense_operator(L)
    rhs = (b - boundary_rhs(L, phi)).reshape(-1)
    x_dense = np.linalg.solve(A, rhs)
    x = phi[1:-1, 1:-1, 1:-1].reshape(-1)
    r = np.abs(rhs - A @ x).max()
    r_dense = np.abs(rhs - A @ x_dense).max()
    gamma = 16.0 * U52 * (np.abs(A) @ np.abs(x)).max()
    ainv = np.abs(np.linalg.inv(A)).sum(axis=1).max()
    return np.abs(x - x_dense).max(), ainv * (r + r_dense + gamma)


def grad_phi(phi, dx, mag=None):
    """k_grad_phi: g (3, nz, ny, nx) of the one-ghost array phi"""
    pc, xm, xp, ym, yp, zm, zp = _neighbours(phi)
    nz, ny, nx = pc.shape
    L = Level((nx, ny, nz), dx)
    faces, _ = _faces(L)
    g = np.zeros((3,) + pc.shape)
    for d, (lo, hi) in enumerate(((xm, xp), (ym, yp), (zm, zp))):
        dl, dh = pc - lo, hi - pc
        dl = np.where(faces[2 * d], 2.0 * dl, dl)
        dh = np.where(faces[2 * d + 1], 2.0 * dh, dh)
        gl, gh = dl / dx[d], dh / dx[d]
        g[d] = -(0.5 * (gl + gh))
        if mag is not None:
            mag[d] = 0.5 * (np.abs(gl) + np.abs(gh))
    return g


def grav_bc_fill(grav, box, geom):
    """castro_amd_grav_bc_fill_fab on grav (3, nz, ny, nx) of `box`, in place: first-order extrapolation beyond inflow / outflow
    faces, reflection (normal component negated) beyond Symmetry faces and walls; periodic directions are left alone"""
    src = grav.copy()
    shape = grav.shape[1:]
    idx, flip, outside = [], [], np.zeros(shape, dtype=bool)
    for d in range(3):
        n = shape[2 - d]
        i = np.arange(box[0][d], box[0][d] + n)
        s = i.copy()
        f = np.zeros(n, dtype=bool)
        out = np.zeros(n, dtype=bool)
        klo = 0 if geom.lo_bc[d] == 0 else (2 if geom.lo_bc[d] >= 3 else 1)
        khi = 0 if geom.hi_bc[d] == 0 else (2 if geom.hi_bc[d] >= 3 else 1)
        below, above = (i < geom.domlo[d]) & (klo != 0), (i > geom.domhi[d]) & (khi != 0)
        s[below] = geom.domlo[d] if klo == 1 else 2 * geom.domlo[d] - i[below] - 1
        s[above] = geom.domhi[d] if khi == 1 else 2 * geom.domhi[d] - i[above] + 1
        f[below], f[above] = klo == 2, khi == 2
        out = below | above
        sh = [1, 1, 1]
        sh[2 - d] = n
        idx.append((s - box[0][d]).reshape(sh) + np.zeros(shape, dtype=np.int64))
        flip.append(f.reshape(sh) | np.zeros(shape, dtype=bool))
        outside |= out.reshape(sh)
    for n in range(3):
        v = src[n][idx[2], idx[1], idx[0]]
        v = np.where(flip[n], -v, v)
        grav[n][outside] = v[outside]


# ---- the backend -----------------------------------------------------------------------------------------------------------------
class PoissonOracleBackend(MR.MonopoleOracleBackend):
    """MonopoleOracleBackend + the Poisson methods, in numpy.  scale: the moments are multiplied by it (the sensitivity probe of
    the driver test takes 1 + 2**-52)."""

    def __init__(self, nthreads=1, scale=1.0):
        super().__init__(nthreads)
        self.scale = float(scale)

    def multipole_moments_mf(self, boxes, geom, mp, out, stream=None):
        specs, _ = boxes
        rb = [(S.numpy()[(URHO,) + MR._sl(sbox, lo, hi)], lo, None if mask is None else mask.numpy())
              for lo, hi, (S, sbox), mask in specs]
        q, _ = moments(rb, geom, mp)
        out.numpy()[:] = q * self.scale

    def multipole_phi_bc(self, phi, phi_box, geom, mp, moments_, stream=None):
        phi_bc(moments_.numpy(), geom, mp, phi.numpy()[0], phi_box)

    def poisson_plan_create(self, geom):
        n = tuple(geom.domhi[d] - geom.domlo[d] + 1 for d in range(3))
        return (n, tuple(geom.dx[d] for d in range(3)))

    def poisson_plan_destroy(self, plan):
        pass

    def poisson_solve(self, plan, phi, phi_box, rho, rho_box, rho_comp, fourpiG, reltol=1.e-10, abstol=1.e-10, maxiter=40,
                      stream=None):
        n, dx = plan
        lo = tuple(x + 1 for x in phi_box[0])
        hi = tuple(x - 1 for x in phi_box[1])
        r = rho.numpy()[(rho_comp,) + MR._sl(rho_box, lo, hi)]
        return solve(n, dx, phi.numpy()[0], r, fourpiG, reltol, abstol, maxiter)

    def grad_phi_to_grav(self, phi, phi_box, grav, grav_box, geom, stream=None):
        lo = tuple(x + 1 for x in phi_box[0])
        hi = tuple(x - 1 for x in phi_box[1])
        g = grav.numpy()
        g[(slice(None),) + MR._sl(grav_box, lo, hi)] = grad_phi(phi.numpy()[0], [geom.dx[d] for d in range(3)])

    def grav_bc_fill(self, grav, grav_box, geom, stream=None):
        grav_bc_fill(grav.numpy(), grav_box, geom)


# ---- the dust-collapse driver case shared by the CPU and the GPU tests: Exec/gravity_tests/DustCollapse/inputs_3d_poisson_regtest
# on 16^3 zones -- the full star, Outflow on all six faces ---------------------------------------------------------------------
DUST_N, DUST_STEPS = (16, 16, 16), 3
DUST_GEOM = dict(prob_lo=(0., 0., 0.), prob_hi=(1.5e9, 1.5e9, 1.5e9), lo_bc=(2, 2, 2), hi_bc=(2, 2, 2))
DUST_CENTER = (7.5e8, 7.5e8, 7.5e8)
DUST_PROB, DUST_PARAMS = MR.DUST_PROB, MR.DUST_PARAMS


def dust_collapse_run(hydro, params, do_grav=True, steps=DUST_STEPS, lnum=0, n_cell=DUST_N, **kw):
    """(driver, [dt of every step]) of the dust-collapse case with Poisson gravity on `hydro`"""
    import castro_amd
    pg = castro_amd.PoissonGravity(max_multipole_order=lnum) if do_grav else None
    c = castro_amd.Castro(n_cell, params=params, hydro=hydro, do_grav=do_grav, poisson=pg, **DUST_GEOM, **kw)
    c.center = DUST_CENTER
    c.initData("dust_collapse", **DUST_PROB)
    return c, [c.step() for _ in range(steps)]


def assert_plan_lifetime(c):
    """a PoissonGravity bound to the Castro `c`, which has made a step: exactly one plan, none after close(), one again after the
    next step"""
    plans = lambda: [e["plan"] for e in c.poisson._lev.values() if e["plan"] is not None]
    assert list(c.poisson._lev) == [0] and len(plans()) == 1 and c.poisson.plan is plans()[0]
    c.close()
    assert plans() == [] and c.poisson.plan is None
    c.close()                                   # idempotent
    c.step()
    assert len(plans()) == 1 and c.poisson.plan is plans()[0] and c.poisson_stats()["new"] is not None


def dust_sensitivity(oracle):
    """(reference driver, its dts, s): the run on PoissonOracleBackend and the deviation per field of a second run whose moments
    are scaled by 1 + 2**-52 (monopole_ref.dust_sensitivity's convention): the tolerance of a comparison is max(1e-10, 100 s)"""
    ref, dts = dust_collapse_run(PoissonOracleBackend(), oracle.default_params(**DUST_PARAMS))
    ulp, _ = dust_collapse_run(PoissonOracleBackend(scale=1.0 + U52), oracle.default_params(**DUST_PARAMS))
    s = MR.field_deviation(ulp.S_new().numpy(), ref.S_new().numpy())
    return ref, dts, s

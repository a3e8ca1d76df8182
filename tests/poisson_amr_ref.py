"""numpy restatement of Poisson gravity on the levels of CastroAmr (tests only): the coarse-fine boundary potential of a level solve
(castro_amd_poisson_cf_bc_fab, written from the comment in include/castro_hydro_amd.h, operation by operation), FillCoarsePatch
of a level that does not solve, the moments and the boundary potential in the device's order of operations (device_order_sum,
phi_bc), a CPU backend that adds poisson_cf_bc and these two to tests/poisson_ref.PoissonOracleBackend, and the
dust-collapse hierarchies the CPU and the GPU driver tests share.  The product never imports this file.

The face formula.  With c = oma * old + a * new (oma = 1.0 - a, one rounding; two products, one sum: 3 roundings per coarse zone),
m = 0.5 * (c_out + c_in) (1 rounding, the factor is exact) and
value = (m0 + s1 * (0.125 * (m1p - m1m))) + s2 * (0.125 * (m2p - m2m)) (2 differences, 2 sums; the factors are exact) a face value
is made with CF_ROUNDINGS = 10 * 3 + 5 + 2 + 2 = 39 roundings, so it lies within 39 * 2**-53 * (the sum of the magnitudes of its terms,
face_values(..., mag=True)) of the same expression in exact arithmetic."""
import numpy as np

from tests import monopole_ref as MR
from tests import poisson_ref as R
from tests.reflux_sources_ref import RegToFlux

CF_ROUNDINGS = 39
U53 = 2.0 ** -53


def _sub(F, box, lo, hi):
    """view of the region [lo, hi] of the array F (nz, ny, nx) that covers `box`"""
    return F[tuple(slice(lo[d] - box[0][d], hi[d] - box[0][d] + 1) for d in (2, 1, 0))]


def _face(m, n1, n2, mag=False):
    """m[T2', T1']: the face means over the coarsened face grown by one (T2 the higher transverse direction); the values of the
    n2 x n1 fine zones of the face.  mag: every term with a plus sign (m holds magnitudes)"""
    i1, i2 = np.arange(n1), np.arange(n2)
    T1, T2 = i1 // 2 + 1, i2 // 2 + 1
    s1 = np.where(i1 & 1, 1.0, -1.0)[None, :]
    s2 = np.where(i2 & 1, 1.0, -1.0)[:, None]
    M = m[np.ix_(T2, T1)]
    if mag:
        return (M + 0.125 * (m[np.ix_(T2, T1 + 1)] + m[np.ix_(T2, T1 - 1)])) + 0.125 * (m[np.ix_(T2 + 1, T1)] + m[np.ix_(T2 - 1, T1)])
    d1 = 0.125 * (m[np.ix_(T2, T1 + 1)] - m[np.ix_(T2, T1 - 1)])
    d2 = 0.125 * (m[np.ix_(T2 + 1, T1)] - m[np.ix_(T2 - 1, T1)])
    return (M + s1 * d1) + s2 * d2


def face_values(crse_old, cobox, crse_new, cnbox, fine_lo, fine_hi, a, mag=False):
    """the shell of the fine box as an array (nz + 2, ny + 2, nx + 2): the six faces hold the boundary values, edges and corners 0,
    the inside NaN.  crse_old / crse_new: (nz, ny, nx) arrays over cobox / cnbox.  mag: the sums of the magnitudes of the terms"""
    clo = tuple((x >> 1) - 1 for x in fine_lo)
    chi = tuple((x >> 1) + 1 for x in fine_hi)
    O, N = _sub(crse_old, cobox, clo, chi), _sub(crse_new, cnbox, clo, chi)
    oma = 1.0 - a
    C = np.abs(oma * O) + np.abs(a * N) if mag else oma * O + a * N
    n = tuple(fine_hi[d] - fine_lo[d] + 1 for d in range(3))
    out = np.full((n[2] + 2, n[1] + 2, n[0] + 2), np.nan)
    for d in range(3):
        ax = 2 - d
        n1, n2 = [n[e] for e in range(3) if e != d]
        for side in (0, 1):
            c_out = np.take(C, 0 if side == 0 else C.shape[ax] - 1, axis=ax)
            c_in = np.take(C, 1 if side == 0 else C.shape[ax] - 2, axis=ax)
            m = 0.5 * (c_out + c_in)
            v = _face(m, n1, n2, mag)
            sl = [slice(1, -1)] * 3
            sl[ax] = 0 if side == 0 else out.shape[ax] - 1
            out[tuple(sl)] = v
    inside = np.zeros(out.shape, dtype=bool)
    inside[1:-1, 1:-1, 1:-1] = True
    out[np.isnan(out) & ~inside] = 0.0                                  # edges and corners
    return out


def cf_bc(phi, phi_box, fine_lo, fine_hi, crse_old, cobox, crse_new, cnbox, a):
    """castro_amd_poisson_cf_bc_fab on phi (nz, ny, nx) of phi_box, in place"""
    sh = face_values(crse_old, cobox, crse_new, cnbox, fine_lo, fine_hi, a)
    dst = _sub(phi, phi_box, tuple(x - 1 for x in fine_lo), tuple(x + 1 for x in fine_hi))
    w = ~np.isnan(sh)
    dst[w] = sh[w]


def fill_coarse_patch(backend, crse_old, crse_new, cbox_data, fine, fbox, a, ncomp):
    """FillCoarsePatch of the whole FAB `fine` (torch, ncomp components, box fbox) from the coarse old / new FABs (torch, box
    cbox_data): the time combination over the coarse zones under fbox grown by one, then cc_interp -- the backend's operations"""
    import torch
    cb = (tuple((x >> 1) - 1 for x in fbox[0]), tuple((x >> 1) + 1 for x in fbox[1]))
    lo = tuple(max(cb[0][d], cbox_data[0][d]) for d in range(3))
    hi = tuple(min(cb[1][d], cbox_data[1][d]) for d in range(3))
    tmp = torch.zeros((ncomp,) + tuple(cb[1][d] - cb[0][d] + 1 for d in (2, 1, 0)), dtype=torch.float64)
    backend.lincomb(tmp, cb, 1.0 - a, crse_old, cbox_data, a, crse_new, cbox_data, ncomp, lo, hi)
    backend.cc_interp(tmp, cb, fine, fbox, fbox[0], fbox[1], ncomp)


MP_WG, MP_MAX_WG, MP_FINAL_GROUPS = 256, 1024, 16


def device_order_sum(term_boxes):
    """The sum of the terms of one moment in the order of k_mp_partial / k_mp_final (the header comments of
    castro_amd/csrc/poisson_kernels.hip): term_boxes holds one array per box, its zones x fastest.  A thread adds the terms of
    its zones base + it * 256 in that order, the 64 lanes of a wave are added pairwise (32, 16, ... 1), the four waves in wave order;
    then group g adds the rows g, g + 16, ... in row order and the 16 groups are added in group order.  Adding 0.0 for a zone a
    thread does not have changes no bits."""
    iters = 1
    while True:
        nwg = [-(-len(t) // (MP_WG * iters)) for t in term_boxes]
        if sum(nwg) <= MP_MAX_WG or iters >= (1 << 20):
            break
        iters *= 2
    rows = []
    for t, n in zip(term_boxes, nwg):
        pad = np.zeros(n * MP_WG * iters)
        pad[:len(t)] = t
        pad = pad.reshape(n, iters, MP_WG)
        acc = np.zeros((n, MP_WG))
        for it in range(iters):
            acc = acc + pad[:, it, :]
        v = acc.reshape(n, MP_WG // 64, 64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v[..., :off] + v[..., off:2 * off]
        w = v[..., 0]
        rows.append(((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])
    rows = np.concatenate(rows)
    sg = []
    for g in range(MP_FINAL_GROUPS):
        acc = 0.0
        for r in range(g, len(rows), MP_FINAL_GROUPS):
            acc = acc + float(rows[r])
        sg.append(acc)
    s = sg[0]
    for g in range(1, MP_FINAL_GROUPS):
        s = s + sg[g]
    return s


def phi_bc(q, geom, mp, phi, box):
    """castro_amd_multipole_phi_bc_fab on phi (nz, ny, nx) of `box`, in place, in the kernel's order of operations
    (k_mp_phi_bc): poisson_ref.phi_bc with the r^(-1) of the l = 0 term formed as the kernel forms it, 1.0 / r -- one correctly
    rounded division.  With lnum = 0 nothing goes through a library function (sqrt and / are correctly rounded on both sides):
    the device's bits.  For l >= 1 pow, and for m >= 1 atan2 / cos / sin, are numpy's, as in poisson_ref."""
    lnum, shape = mp.lnum, phi.shape
    loc, outside = [], np.zeros(shape, dtype=bool)
    for d, n in enumerate(shape[::-1]):
        idx = np.arange(box[0][d], box[0][d] + n)
        f = idx.astype(np.float64)
        v = np.where(idx > geom.domhi[d], geom.problo[d] + f * geom.dx[d] - mp.center[d],
                     np.where(idx < geom.domlo[d], geom.problo[d] + (f + 1.0) * geom.dx[d] - mp.center[d],
                              geom.problo[d] + (f + 0.5) * geom.dx[d] - mp.center[d])) / mp.rmax
        sh = [1, 1, 1]
        sh[2 - d] = n
        loc.append(v.reshape(sh) + np.zeros(shape))
        outside |= ((idx < geom.domlo[d]) | (idx > geom.domhi[d])).reshape(sh)
    x, y, z = loc
    r = np.sqrt(x * x + y * y + z * z)
    rmax_cubed = mp.rmax * mp.rmax * mp.rmax
    with np.errstate(all="ignore"):
        cosT, phiA = z / r, np.arctan2(y, x)
        acc = np.zeros(shape)
        st = [None, None, None]
        for l in range(lnum + 1):
            R.leg_step(l, st, cosT)
            r_U = 1.0 / r if l == 0 else np.power(r, float(-l - 1))
            acc = acc + q[R.qindex(lnum, 0, l, 0)] * st[0] * r_U * rmax_cubed
        for m in range(1, lnum + 1):
            st = [None, None, None]
            for l in range(m, lnum + 1):
                R.assoc_step(l, m, st, cosT)
                r_U = np.power(r, float(-l - 1))
                amp = q[R.qindex(lnum, 1, l, m)] * np.cos(m * phiA) + q[R.qindex(lnum, 2, l, m)] * np.sin(m * phiA)
                acc = acc + amp * st[0] * r_U * rmax_cubed
        val = np.where(r < 1.0e-12, 0.0, -mp.Gconst * acc / mp.rmax)
    phi[outside] = val[outside]


class PoissonAmrOracleBackend(RegToFlux, R.PoissonOracleBackend):
    """PoissonOracleBackend + poisson_cf_bc, in numpy (and the register-to-flux operation of update_sources_after_reflux).  The
    moments are summed in the device's order (device_order_sum) instead of exactly, and the boundary potential takes r^(-1) as the
    kernel does (phi_bc above): with max_multipole_order = 0, where pow(r, 0) = 1, both are the device's bits."""

    def multipole_phi_bc(self, phi, phi_box, geom, mp, moments_, stream=None):
        phi_bc(moments_.numpy(), geom, mp, phi.numpy()[0], phi_box)

    def multipole_moments_mf(self, boxes, geom, mp, out, stream=None):
        specs, _ = boxes
        per_key = {}
        for lo, hi, (S, sbox), mask in specs:
            assert mask is None, "device_order_sum: masked boxes are not restated"
            rho = S.numpy()[(R.URHO,) + MR._sl(sbox, lo, hi)]
            for key, (t, _) in R.moment_terms([(rho, lo, None)], geom, mp).items():
                per_key.setdefault(key, []).append(t)
        n1 = mp.lnum + 1
        q = np.zeros(3 * n1 * n1)
        for (kind, l, m), tb in per_key.items():
            q[R.qindex(mp.lnum, kind, l, m)] = device_order_sum(tb)
        out.numpy()[:] = q * self.scale

    def poisson_cf_bc(self, phi, phi_box, fine_lo, fine_hi, crse_old, crse_old_box, crse_new, crse_new_box, a, stream=None):
        cf_bc(phi.numpy()[0], phi_box, fine_lo, fine_hi, crse_old.numpy()[0], crse_old_box, crse_new.numpy()[0], crse_new_box, a)


# ---- the dust-collapse hierarchies shared by the CPU and the GPU tests: poisson_ref's DUST_* case (the full star in 16^3 zones)
# with a fixed 16^3 patch over the coarse zones 4..11, and with a second 16^3 patch over the zones 12..19 of level 1 -----------------
AMR_N, AMR_STEPS = (16, 16, 16), 2
PATCH1 = ((4, 4, 4), (11, 11, 11))
PATCH2 = ((12, 12, 12), (19, 19, 19))
CASES = {"one": [PATCH1], "two": [PATCH1, PATCH2]}


def dust_amr_run(make_hydro, params, case="one", steps=AMR_STEPS, max_solve_level=None, **kw):
    """(hierarchy, [dt of every coarse step]) of the dust collapse with Poisson gravity on a refined hierarchy"""
    import castro_amd
    if "refine" not in kw:
        kw["patches"] = CASES[case]
    pg = castro_amd.PoissonGravity(center=R.DUST_CENTER, max_solve_level=max_solve_level)
    a = castro_amd.CastroAmr(AMR_N, params=params, make_hydro=make_hydro, do_grav=True, gravity=pg, **R.DUST_GEOM, **kw)
    a.initData("dust_collapse", **R.DUST_PROB)
    return a, [a.step() for _ in range(steps)]


def single_and_hierarchy(make_hydro, params, steps=2):
    """(Castro(poisson=...), CastroAmr(gravity=...) with no refined level) after `steps` steps of the dust collapse from the same
    state, lnum = 2"""
    import castro_amd
    c = castro_amd.Castro(AMR_N, params=params, hydro=make_hydro(), do_grav=True, poisson=castro_amd.PoissonGravity(max_multipole_order=2),
                          **R.DUST_GEOM)
    c.center = R.DUST_CENTER
    a = castro_amd.CastroAmr(AMR_N, params=params, make_hydro=make_hydro, do_grav=True, patches=[],
                             gravity=castro_amd.PoissonGravity(max_multipole_order=2, center=R.DUST_CENTER), **R.DUST_GEOM)
    c.initData("dust_collapse", **R.DUST_PROB)
    a.initData("dust_collapse", **R.DUST_PROB)
    a.lev[0].boxes[0].S_new_b.copy_(c.S_new_b)
    for _ in range(steps):
        c.step()
        a.step()
    return c, a


def assert_routes_agree(c, a):
    """the two routes to the field of a single level leave the same bits: S_new, phi of both time levels with the ghost shell,
    grav_old / grav_new with their ghost zones, and the statistics of the solves"""
    bits = lambda t: t.cpu().numpy().view(np.int64)
    b = a.lev[0].boxes[0]
    assert len(a.lev) == 1 and c.nstep == a.nstep == 2 and c.time == a.time
    for name in ("S_new_b", "grav_old", "grav_new"):
        assert np.array_equal(bits(getattr(c, name)), bits(getattr(b, name))), name
    for new in (True, False):
        assert np.array_equal(bits(c.phi_grav(new)), bits(a.phi_grav(0, new))), new
    assert c.phi_grav().shape == (1, 18, 18, 18) and float(c.phi_grav().abs().max()) > 0.0
    st = c.poisson_stats()
    assert st == a.poisson_stats(0) and st["first"]["cycles"] > 0 and st["new"] is not None and st["old"] is not None


def level_fields(a):
    """[(S_new, phi_new, grav_new) of the box of every level] as numpy arrays"""
    out = []
    for l, lev in enumerate(a.lev):
        b = lev.boxes[0]
        out.append((b.S_new().cpu().numpy().copy(), a.phi_grav(l).cpu().numpy().copy(), b.grav_new.cpu().numpy().copy()))
    return out


def dust_amr_sensitivity(oracle, case):
    """(reference hierarchy, its dts, s per level): the run on PoissonAmrOracleBackend and the deviation per field of a second run
    whose moments are scaled by 1 + 2**-52 (the rule of poisson_ref.dust_sensitivity)"""
    P = lambda: oracle.default_params(**R.DUST_PARAMS)
    ref, dts = dust_amr_run(lambda: PoissonAmrOracleBackend(), P(), case)
    ulp, _ = dust_amr_run(lambda: PoissonAmrOracleBackend(scale=1.0 + R.U52), P(), case)
    s = [MR.field_deviation(u[0], r[0]) for u, r in zip(level_fields(ulp), level_fields(ref))]
    return ref, dts, s

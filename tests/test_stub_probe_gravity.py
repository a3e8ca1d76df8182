"""The restatements of monopole gravity, the point mass and the multipole boundary against
tests/golden/stub_probe/gravity_vectors.npz: outputs of the reference's own Gravity::install_level, compute_radial_mass,
make_radial_gravity, interpolate_monopole_grav, add_pointmass_to_gravity, init_multipole_grav and fill_multipole_BCs, compiled
unmodified against stand-in headers (tools/stub_probe/probe_gravity.cpp; STUB-COMPILED, NOT oracle/_ref).  Only the fixture is
read.  tests/test_stub_probe_gravity_gpu.py replays the same cases through the device entry points.

Bit for bit: the bin and the count of every sub-zone, n1d, max_radius_all_in_domain, the combined profiles, radial_grav, the
interpolated gravity, the point-mass terms, rmax, the r < 1e-12 zeros, the untouched interior of phi -- and, because the probe
runs on one thread, radial_mass and radial_vol themselves against the loop-nest sums of monopole_ref.radial_mass (seq, vol_seq).
Within the bounds the project already grants: the exactly rounded bin masses (mass_bounds), the moments and the boundary
potential (the allowances of tests/poisson_ref.py).  Derived here: radial_vol against count * vol_frac, which is what the device
forms: count additions of vol_frac are within count * 2**-53 * (count * vol_frac) of the product.

The file also asserts that the fixture holds every branch it is there for (test_the_fixture_holds_every_branch)."""
import math

import numpy as np
import pytest

from castro_amd import _lib
from tests import monopole_amr_ref as AR
from tests import monopole_ref as R
from tests import pointmass_ref as PR
from tests import poisson_ref as Q
from tests import stub_probe_gravity as V

_REF = {}
WORST = {}


def _worst(family, value):
    WORST[family] = max(WORST.get(family, 0.0), float(value))


def _ratio(err, bound):
    assert np.all(err[bound == 0.0] == 0.0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def vol_bound(ref):
    """|count additions of vol_frac - count * vol_frac| <= count * 2**-53 * (count * vol_frac), per bin"""
    return ref["count"].astype(np.float64) * 2.0 ** -53 * ref["vol"]


def check_bins(ref, want_mass, want_vol, geom, mono, what):
    """recorded radial_mass / radial_vol of one level against the dict of monopole_ref.radial_mass"""
    vf = R.vol_frac(geom, mono)
    assert np.array_equal(np.rint(want_vol / vf).astype(np.int64), ref["count"]), what + ": the count of every bin"
    assert V.same(want_vol, ref["vol_seq"]), what + ": radial_vol, one addition per sub-zone in loop order"
    assert V.same(want_mass, ref["seq"]), what + ": radial_mass in loop order"
    eb, em = np.abs(want_vol - ref["vol"]), np.abs(want_mass - ref["mass"])
    assert np.all(eb <= vol_bound(ref)) and np.all(em <= R.mass_bounds(ref)), what
    _worst("radial_vol vs count * vol_frac / bound", _ratio(eb, vol_bound(ref)))
    _worst("radial_mass vs fsum / mass_bounds", _ratio(em, R.mass_bounds(ref)))
    return bool(np.all(eb == 0.0) and np.all(em == 0.0))


def rm_ref(i):
    if ("rm", i) not in _REF:
        c = V.radial_mass_case(i)
        _REF[("rm", i)] = (c, R.radial_mass([(rho, b[0], None) for rho, b in zip(c.rho, c.bx)], c.geom, c.mono))
    return _REF[("rm", i)]


@pytest.mark.parametrize("i", V.case_ids("rm"))
def test_compute_radial_mass(i):
    c, ref = rm_ref(i)
    exact = check_bins(ref, c.want_mass, c.want_vol, c.geom, c.mono, c.P)
    dyadic = all(math.frexp(x)[0] in (0.5, 0.625, 0.75, 0.875) for x in c.dx)
    if dyadic:
        assert exact, "dyadic inputs: every sum is exact in any order"
    # the octant factor is in the recorded volumes
    per = c.want_vol.sum() / ref["count"].sum() / ((c.dx[0] / c.drdxfac) * (c.dx[1] / c.drdxfac) * (c.dx[2] / c.drdxfac))
    assert abs(per - R.octant_factor(c.geom, c.mono)) < 1e-9


def level_rho(c, l):
    """[(rho the reference bins, lo, mask)] of level l and the time branch"""
    branch, oa, al = V.time_branch(c.time, *c.times[l])
    out = []
    for b, bx in enumerate(c.boxes[l]):
        rho = {"old": c.rho_old[l][b], "new": c.rho_new[l][b], "same": c.rho_new[l][b]}.get(branch)
        if rho is None:
            rho = AR.interp_rho(c.rho_old[l][b], c.rho_new[l][b], oa, al)
        m = c.mask[l][b] if l < c.level else None
        out.append((rho, bx[0], None if m is None else (m != 0.0).astype(np.uint8)))
    return branch, out


def rg_ref(i):
    if ("rg", i) not in _REF:
        c = V.radial_gravity_case(i)
        refs = []
        for l in range(c.level + 1):
            branch, boxes = level_rho(c, l)
            if branch == "mix":
                _, oa, al = V.time_branch(c.time, *c.times[l])
                ref = AR.radial_mass_ex([(c.rho_old[l][b], c.rho_new[l][b], bx[0], boxes[b][2], oa, al) for b, bx in enumerate(c.boxes[l])],
                                        c.geoms[l], c.monos[l])
            else:
                ref = R.radial_mass(boxes, c.geoms[l], c.monos[l])
            refs.append(ref)
        _REF[("rg", i)] = (c, refs)
    return _REF[("rg", i)]


@pytest.mark.parametrize("i", V.case_ids("rg"))
def test_make_radial_gravity(i):
    c, refs = rg_ref(i)
    # install_level: the bins of every level and the radius
    for l in range(c.level + 1):
        assert c.want_n1d[l] == c.drdxfac * c.numpts[l]
        if c.numpts[l] == int(math.sqrt(float(sum(x * x for x in c.n_cell[l])))) + 2 * _lib.NUM_GROW:
            assert c.want_n1d[l] == _lib.monopole_n1d(c.n_cell[l], c.drdxfac)
        assert c.monos[l].max_radius_all_in_domain == c.want_maxrad
        check_bins(refs[l], c.want_mass[l], c.want_vol[l], c.geoms[l], c.monos[l], "%slevel %d" % (c.P, l))
    # the level combination and the integration on the recorded arrays: a fixed order, so the same bits
    arrays = [(c.want_mass[l], c.want_vol[l]) for l in range(c.level + 1)]
    m, v = AR.combine(arrays, c.want_n1d, c.level)
    grav = R.radial_gravity(m, v, c.geoms[c.level], c.monos[c.level])
    assert V.same(grav, c.want_grav), "%d bins of radial_grav differ" % int((grav != c.want_grav).sum())
    # what the device's volumes (count * vol_frac) do to radial_grav: measured, and bounded by what they do to the density
    m2, v2 = AR.combine([(c.want_mass[l], refs[l]["vol"]) for l in range(c.level + 1)], c.want_n1d, c.level)
    g2 = R.radial_gravity(m2, v2, c.geoms[c.level], c.monos[c.level])
    dev = np.abs(g2 - c.want_grav).max() / np.abs(c.want_grav).max()
    _worst("radial_grav from count * vol_frac, of its largest magnitude", dev)
    print("%sradial_grav from count * vol_frac volumes: %.3g of the largest magnitude" % (c.P, dev))
    assert dev <= 4.0 * 2.0 ** -53 * c.want_n1d[c.level], "one rounding of the density per outer bin, accumulated"


@pytest.mark.parametrize("i", V.case_ids("ig"))
def test_interpolate_monopole_grav(i):
    c = V.interpolate_case(i)
    for b, gbox in enumerate(c.gbox):
        grav = np.full(c.want[b].shape, c.fill)
        R.interpolate(c.rg, c.geom, c.mono, grav, gbox)
        assert V.same(grav, c.want[b]), "%sbox %d: %d values differ" % (c.P, b, int((grav != c.want[b]).sum()))


def phi_term(box, geom, center, Gconst, M):
    """what add_pointmass_to_gravity subtracts from phi on `box`: C::Gconst * point_mass * rinv (Gravity.cpp:2926-2940)"""
    lo, hi = box
    r = [geom.problo[d] + (np.arange(lo[d], hi[d] + 1).astype(np.float64) + 0.5) * geom.dx[d] - center[d] for d in range(3)]
    x, y, z = r[0][None, None, :], r[1][None, :, None], r[2][:, None, None]
    rsq = x * x + y * y + z * z
    return Gconst * M * (1.e0 / np.sqrt(rsq))


@pytest.mark.parametrize("i", V.case_ids("pg"))
def test_add_pointmass_to_gravity(i):
    c = V.pointmass_case(i)
    for b, gbox in enumerate(c.gbox):
        grav = c.grav[b].copy()
        PR.add_pointmass(grav, gbox, c.geom, c.center, _lib.GCONST, c.mass)
        assert V.same(grav, c.want_grav[b].reshape(grav.shape)), "%sbox %d" % (c.P, b)
        term = PR.pointmass_term(gbox, c.geom, c.center, _lib.GCONST, c.mass)
        assert np.all(np.abs(term).sum(axis=0) > 0.0)
        phi = c.phi[b] - phi_term(c.pbox[b], c.geom, c.center, _lib.GCONST, c.mass)
        assert V.same(phi, c.want_phi[b]), "%sphi of box %d: written on its own box only" % (c.P, b)


def mp_moments(c):
    """(q, bound) over the levels: level l < finest masked by the level above, the parts added in level order"""
    q, bound = None, None
    for l in range(c.nlev):
        mp = _lib.make_multipole(c.geoms[0], c.center, c.lnum)
        boxes = [(c.rho[l][b], bx[0], None if c.mask[l][b] is None else (c.mask[l][b] != 0.0).astype(np.uint8))
                 for b, bx in enumerate(c.boxes[l])]
        ql, bl = Q.moments(boxes, c.geoms[l], mp)
        if q is None:
            q, bound = ql, bl
        else:
            bound = bound + bl + Q.U52 * (np.abs(q) + np.abs(ql))
            q = q + ql
    return q, bound


def want_q(c):
    n1 = c.lnum + 1
    return np.concatenate([np.pad(c.want_qL0.reshape(n1, 1), ((0, 0), (0, n1 - 1))).ravel(), c.want_qLC, c.want_qLS])


@pytest.mark.parametrize("i", V.case_ids("mp"))
def test_multipole_boundary(i):
    c = V.multipole_case(i)
    mp = _lib.make_multipole(c.geoms[0], c.center, c.lnum)
    n1 = c.lnum + 1
    # init_multipole_grav: rmax, no Symmetry face -> every factor 1, nothing mirrored, factArray = 2 (l - m)! / (l + m)!
    assert mp.rmax == float(c.want_rmax[0]) and c.want_volumeFactor[0] == 1.0
    assert np.all(c.want_parity_q0 == 1.0) and np.all(c.want_parity_qC_qS == 1.0) and np.all(c.want_symmetric == 0.0)
    fa = np.array([[Q.fact_array(l, m) if 1 <= m <= l else 0.0 for m in range(n1)] for l in range(n1)])
    assert V.same(fa.ravel(), c.want_factArray)
    for l in range(c.nlev):
        g = c.geoms[l]
        assert g.dx[0] * g.dx[1] * g.dx[2] == c.want_vol[l]
    # the zone loop
    q, bound = mp_moments(c)
    want = want_q(c)
    err = np.abs(q - want)
    assert np.all(err <= bound), "%sworst moment deviation / allowance %.3g" % (c.P, _ratio(err, bound))
    _worst("moments / allowance", _ratio(err, bound))
    # the boundary loop, from the recorded moments
    phi = c.phi.copy()
    outside, allow = Q.phi_bc(want, c.geoms[0], mp, phi, c.pbox)
    assert V.same(phi[~outside], c.want_phi[~outside]) and V.same(c.want_phi[~outside], c.phi[~outside]), "the interior is untouched"
    assert outside.sum() == phi.size - (phi.shape[0] - 2) * (phi.shape[1] - 2) * (phi.shape[2] - 2)
    err = np.abs(phi - c.want_phi)
    assert np.all(err <= allow), "%sworst phi deviation / allowance %.3g" % (c.P, _ratio(err[outside], allow[outside]))
    _worst("phi_bc / allowance", _ratio(err[outside], allow[outside]))
    zero = c.want_phi == 0.0
    assert V.same(phi[zero], c.want_phi[zero]), "the r < 1e-12 zone holds +0.0"
    if tuple(c.center) == tuple(c.problo):
        assert zero[0, 0, 0] and zero.sum() == 1


def test_the_fixture_holds_every_branch():
    """a regenerated fixture cannot quietly lose a case"""
    # compute_radial_mass: both octant outcomes, the three near misses of the threshold, every class of zone at a short n1d,
    # zeros of both signs, a sub-zone on a bin edge, one to three boxes, drdxfac 1, 2, 4, both families
    octs, seen = set(), set()
    for i in V.case_ids("rm"):
        c, ref = rm_ref(i)
        o = R.octant_factor(c.geom, c.mono)
        off = [abs(c.center[d] - c.problo[d]) / c.dx[d] for d in range(3)]
        octs.add((o, tuple(round(x, 3) for x in off) if max(off) < 0.02 else None))
        seen.add(("boxes", len(c.bx)))
        seen.add(("drdxfac", c.drdxfac))
        seen.add(("dyadic", all(math.frexp(x)[0] in (0.5, 0.625, 0.75, 0.875) for x in c.dx)))
        if c.level > 0:
            assert ref["dropped"] > 0
            n1d, f = c.n1d, c.drdxfac
            for rho, bx in zip(c.rho, c.bx):
                lo = R._axes(bx[0], rho.shape, c.geom, c.mono, 0.0)
                ce = R._axes(bx[0], rho.shape, c.geom, c.mono, 0.5)
                zb = np.floor(np.sqrt(ce[0] ** 2 + ce[1] ** 2 + ce[2] ** 2) / (c.dx[0] / f)).astype(int)
                sb = []
                for kk in range(f):
                    for jj in range(f):
                        for ii in range(f):
                            xx, yy, zz = (lo[d] + ((ii, jj, kk)[d] + 0.5) * (c.dx[d] / f) for d in range(3))
                            sb.append(np.floor(np.sqrt(xx * xx + yy * yy + zz * zz) / (c.dx[0] / f)).astype(int))
                sb = np.array(sb)
                if ((zb > n1d - 1) & (sb <= n1d - 1).any(axis=0)).any():
                    seen.add("dropped zone with sub-zones inside")
                if ((zb <= n1d - 1) & (sb > n1d - 1).any(axis=0)).any():
                    seen.add("kept zone with sub-zones beyond")
        for rho in c.rho:
            z = rho == 0.0
            if z.any() and np.signbit(rho[z]).any() and (~np.signbit(rho[z])).any():
                seen.add("zeros of both signs")
        if c.dx[0] == c.dx[1] == c.dx[2]:
            lo = R._axes(c.bx[0][0], c.rho[0].shape, c.geom, c.mono, 0.0)
            f = c.drdxfac
            for kk in range(f):
                for jj in range(f):
                    for ii in range(f):
                        xx, yy, zz = (lo[d] + ((ii, jj, kk)[d] + 0.5) * (c.dx[d] / f) for d in range(3))
                        q = np.sqrt(xx * xx + yy * yy + zz * zz) * (1.0 / (c.dx[0] / f))
                        if (q == 5.0).any():
                            seen.add(("bin edge", f))
    assert {(8.0, (0.0, 0.0, 0.0)), (8.0, (0.009, 0.009, 0.009)), (1.0, (0.011, 0.0, 0.0)), (1.0, None)} <= octs, octs
    for k in (("boxes", 1), ("boxes", 2), ("boxes", 3), ("drdxfac", 1), ("drdxfac", 2), ("drdxfac", 4), ("dyadic", True), ("dyadic", False),
              "dropped zone with sub-zones inside", "kept zone with sub-zones beyond", "zeros of both signs", ("bin edge", 1), ("bin edge", 2)):
        assert k in seen, k
    # make_radial_gravity: the four time branches, one to three levels, two boxes on level 1, a masked zone with density, the
    # placings of max_radius_all_in_domain, empty bins on both sides of it and directly below it, rc == max_radius_all_in_domain
    seen = set()
    for i in V.case_ids("rg"):
        c, refs = rg_ref(i)
        seen.add(("levels", c.level + 1))
        for l in range(c.level + 1):
            seen.add(V.time_branch(c.time, *c.times[l])[0])
            if len(c.boxes[l]) == 2 and l == 1:
                seen.add("level 1 in two boxes")
            if l < c.level and any(((m == 0.0) & (ro != 0.0) & (rn != 0.0)).any() for m, ro, rn in zip(c.mask[l], c.rho_old[l], c.rho_new[l])):
                seen.add("masked zone with density")
        branch, oa, al = V.time_branch(c.time, *c.times[c.level])
        if branch == "mix":
            ro, rn = c.rho_old[c.level][0], c.rho_new[c.level][0]
            from fractions import Fraction as F
            once = np.array([float(F(oa) * F(float(x)) + F(al) * F(float(y))) for x, y in zip(ro.ravel(), rn.ravel())])
            if (once != AR.interp_rho(ro, rn, oa, al).ravel()).any():
                seen.add("two roundings visible")
        n1d, mono = c.want_n1d[c.level], c.monos[c.level]
        dr = c.geoms[c.level].dx[0] / c.drdxfac
        rc = (np.arange(n1d) + 0.5) * dr
        inner = rc < c.want_maxrad
        inner[0] = True
        _, v = AR.combine([(c.want_mass[l], c.want_vol[l]) for l in range(c.level + 1)], c.want_n1d, c.level)
        if inner.all():
            seen.add("maxrad beyond the last bin")
        elif not inner[1]:
            seen.add("maxrad below the centre of bin 1")
        elif inner.sum() < n1d - 2:
            seen.add("maxrad mid-array")
        if (v[inner][1:] == 0.0).any():
            seen.add("empty inner bin")
        if (v[~inner] == 0.0).any():
            seen.add("empty outer bin")
        if not inner.all() and inner[1] and v[inner.sum() - 1] == 0.0:
            seen.add("empty bin directly below maxrad")
        if (rc == c.want_maxrad).any():
            seen.add("rc == maxrad")
    for k in (("levels", 1), ("levels", 2), ("levels", 3), "old", "new", "mix", "same", "level 1 in two boxes", "masked zone with density",
              "two roundings visible", "maxrad beyond the last bin", "maxrad below the centre of bin 1", "maxrad mid-array",
              "empty inner bin", "empty outer bin", "empty bin directly below maxrad", "rc == maxrad"):
        assert k in seen, k
    # interpolate_monopole_grav: every class of bin, both clamps, kept sentinels, drdxfac 1 and 2, a zone 1e-3 dx from the centre
    seen = set()
    for i in V.case_ids("ig"):
        c = V.interpolate_case(i)
        seen.add(("drdxfac", c.drdxfac))
        assert c.ng > 0 and c.level > 0
        for b, gbox in enumerate(c.gbox):
            info, grav = {}, np.full(c.want[b].shape, c.fill)
            index = R.interpolate(c.rg, c.geom, c.mono, grav, gbox, info)
            n1d = c.rg.size
            for name, m in (("bin 0", index == 0), ("last bin", index == n1d - 1), ("between", (index > 0) & (index < n1d - 1)),
                            ("beyond", index > n1d - 1), ("min clamp", info["clamp"] == -1), ("max clamp", info["clamp"] == 1)):
                if m.any():
                    seen.add(name)
            assert np.all(c.want[b][:, index > n1d - 1] == c.fill) and np.all(c.want[b][:, index <= n1d - 1] != c.fill)
            ce = R._axes(gbox[0], grav.shape[1:], c.geom, c.mono, 0.5)
            r = np.sqrt(ce[0] ** 2 + ce[1] ** 2 + ce[2] ** 2)
            if 0.0 < r.min() < 2.0e-3 * max(c.dx):
                seen.add("1e-3 dx from the centre")
    for k in (("drdxfac", 1), ("drdxfac", 2), "bin 0", "last bin", "between", "beyond", "min clamp", "max clamp", "1e-3 dx from the centre"):
        assert k in seen, k
    # add_pointmass_to_gravity: grav wider than phi, the centre on a corner and inside a zone, masses of both magnitudes
    seen = set()
    for i in V.case_ids("pg"):
        c = V.pointmass_case(i)
        if c.ng_grav > c.ng_phi:
            seen.add("contains")
        off = [(c.center[d] - c.problo[d]) / c.dx[d] for d in range(3)]
        seen.add("corner" if all(abs(x - round(x)) < 1e-9 for x in off) else "inside")
        seen.add("heavy" if c.mass > 1e20 else "light")
        assert not (c.dx[0] == c.dx[1] == c.dx[2])
    assert {"contains", "corner", "inside", "heavy", "light"} <= seen, seen
    # fill_multipole_BCs: lnum 0, 2, 6; one and two levels; both domains; the three placings; the r < 1e-12 zone
    seen = set()
    for i in V.case_ids("mp"):
        c = V.multipole_case(i)
        seen.update([("lnum", c.lnum), ("levels", c.nlev), ("domain", c.n_cell[0])])
        if c.nlev == 2:
            assert any(((m == 0.0) & (r != 0.0)).any() for m, r in zip(c.mask[0], c.rho[0]))
        mid = tuple(c.problo[d] + 0.5 * c.n_cell[0][d] * c.dx[d] for d in range(3))
        seen.add("corner" if tuple(c.center) == tuple(c.problo) else "mid" if tuple(c.center) == mid else "off")
        if (c.want_phi == 0.0).any():
            seen.add("r < 1e-12")
    for k in (("lnum", 0), ("lnum", 2), ("lnum", 6), ("levels", 1), ("levels", 2), ("domain", (12, 7, 5)), ("domain", (8, 8, 8)), "corner",
              "mid", "off", "r < 1e-12"):
        assert k in seen, k


def test_worst_deviations_are_reported():
    """the worst deviation / bound of each family over the replays above (printed; tools/stub_probe/README.md quotes them)"""
    for k in sorted(WORST):
        print("%s: %.3g" % (k, WORST[k]))
        if k.endswith("bound") or k.endswith("allowance") or k.endswith("mass_bounds"):
            assert WORST[k] <= 1.0

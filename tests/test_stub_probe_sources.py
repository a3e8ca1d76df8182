"""The restatements of the source terms against tests/golden/stub_probe/source_vectors.npz: outputs of the reference's own
Castro::apply_sponge / construct_new_sponge_source (Source/sources/Castro_sponge.cpp), construct_old/new_gravity_source
(Source/gravity/Castro_gravity.cpp, grav_source_type 1-4, one vector everywhere and a FAB that varies from zone to zone) and
Castro::pointmass_update (Source/gravity/Castro_pointmass.cpp), compiled unmodified against stand-in headers
(tools/stub_probe/probe_sources.cpp).  STUB-COMPILED, NOT oracle/_ref.  Only the fixture is read.

Every recorded value is reproduced bit for bit by tests/sponge_ref.py, tests/monopole_ref.py (the gravity-FAB source functions),
oracle/ora_sources.c (the one-vector gravity sources) and tests/pointmass_ref.py, with one allowance: a sponge zone whose factor
went through the ramp's cos -- numpy's cos is not the recording host's libm -- may differ by RAMP_REL of tests/test_sponge_cpu.py,
relative to |Sr_n| for a momentum source and to sum_n |v_n Sr_n| for the energy source (the sum of three products of such
values).  tests/test_stub_probe_sources_gpu.py replays the same cases on the device."""
import types

import numpy as np
import pytest

from oracle import oracle_lib as O
from tests import monopole_ref as R
from tests import pointmass_ref as PR
from tests import sponge_ref as S
from tests import stub_probe_sources as V
from tests.test_sponge_cpu import RAMP_REL


def count(n, exact, allowed, what):
    print("%s: %d recorded values, %d compared bit for bit, %d under the ramp allowance" % (what, n, exact, allowed))


# ---- sponge ----------------------------------------------------------------------------------------------------------------------
def sponge_reference(c):
    """(source of the restatement, info) of a case"""
    info = {}
    got = S.apply_sponge(c.U, c.box, c.lo, c.hi, c.sponge, c.geom, types.SimpleNamespace(eos_gamma=c.eos_gamma, abar=1.0), c.dt, info)
    return got, info


def sponge_branches(c, info):
    """every ramp of the case has zones below, on and above it (a step: none on it), and a ramp case has a zone exactly on a cutoff"""
    sp = c.sponge
    u = c.U
    x = dict(radius=S.radius(sp, c.geom, c.lo, c.hi), density=u[S.URHO], pressure=info["pressure"])
    lim = dict(radius=(sp.lower_radius, sp.upper_radius), density=(sp.lower_density, sp.upper_density),
               pressure=(sp.lower_pressure, sp.upper_pressure))
    assert set(info["region"]) == set(c.ramps), (info["region"].keys(), c.ramps)
    for name, (below, on, above) in info["region"].items():
        assert below.sum() > 0 and above.sum() > 0, (c.P, name, below.sum(), above.sum())
        hit = int((x[name] == lim[name][0]).sum() + (x[name] == lim[name][1]).sum())
        if c.step:
            assert on.sum() == 0 and hit == 0, (c.P, name)
        else:
            assert on.sum() > 0 and hit >= 2, (c.P, name, on.sum(), hit)        # a zone on the lower and one on the upper cutoff
    at_rest = (u[S.UMX] == 0.0) & (u[S.UMY] == 0.0) & (u[S.UMZ] == 0.0)
    assert at_rest.sum() >= 3
    # the zones exactly on a cutoff of the ramp that decides (the last active one: pressure over density over radius)
    last = c.ramps[-1]
    return (x[last] == lim[last][0]) | (x[last] == lim[last][1])


def sponge_allowance(c, want):
    """(4, nz, ny, nx): what UMX, UMY, UMZ, UEDEN of a ramp zone may differ by (module docstring)"""
    v = [np.abs(c.U[S.UMX + n] * (1.0 / c.U[S.URHO])) for n in range(3)]
    m = [np.abs(want[S.UMX + n]) for n in range(3)]
    return RAMP_REL * np.stack(m + [v[0] * m[0] + v[1] * m[1] + v[2] * m[2]])


@pytest.mark.parametrize("c", V.case_ids("sponge"))
def test_sponge_restatement(c):
    c = V.sponge_case(c)
    got, info = sponge_reference(c)
    on_cutoff = sponge_branches(c, info)
    cosm = info["cos"]
    want = c.want
    assert want.shape == got.shape == (S.NSRC,) + c.U.shape[1:]
    alpha0 = not c.timescale > 0.0
    if alpha0:
        assert info["alpha"] == 0.0 and np.all(want == 0.0)
    else:
        assert np.abs(want[S.UMX:S.UMZ + 1]).max() > 0.0
    if c.step:
        assert not cosm.any()
    else:
        assert cosm.any() and (~cosm).any(), "zones of both kinds: the allowance cannot cover the whole case"
    for n in (S.URHO, S.UEINT, S.UTEMP):
        assert np.all(want[n] == 0.0) and np.all(got[n] == 0.0)
    k = [S.UMX, S.UMY, S.UMZ, S.UEDEN]
    g, w = got[k], want[k]
    assert V.same(g[:, ~cosm], w[:, ~cosm]), "%s: %d values outside every ramp differ" % (c.P, V.differing(g[:, ~cosm], w[:, ~cosm]))
    if not c.step:
        # On a cutoff the ramp's argument is 0 or pi, where every cos is exactly 1 or -1: no allowance there.  With the factors of
        # the fixture the far end of the ramp is one ulp off upper_factor, so `<` for the reference's `<=` (Castro_sponge.cpp:125,
        # :144, :181) shows here and nowhere else.
        assert on_cutoff.sum() >= 2 and np.all(cosm[on_cutoff])
        assert V.same(g[:, on_cutoff], w[:, on_cutoff]), "%s: a zone exactly on a cutoff differs" % c.P
    if cosm.any() and not alpha0:
        d, tol = np.abs(g - w)[:, cosm], sponge_allowance(c, want)[:, cosm]
        print("%s: largest |restatement - reference| / allowance in a ramp zone = %.3g, %d of %d ramp values bit-equal"
              % (c.P, (d / np.where(tol > 0, tol, 1.0)).max(), int((d == 0).sum()), d.size))
        assert np.all(d <= tol), (c.P, float((d / np.where(tol > 0, tol, 1.0)).max()))
    else:
        assert V.same(g, w)
    count(want.size, want.size - 4 * int(cosm.sum()) * (not alpha0), 4 * int(cosm.sum()) * (not alpha0), c.P)


# ---- gravity sources -------------------------------------------------------------------------------------------------------------
def gravity_branches(c):
    mo = np.abs(c.uold[1:4]).max(axis=0) == 0.0
    mn = np.abs(c.unew[1:4]).max(axis=0) == 0.0
    assert (mo & ~mn).sum() > 0 and (mo & mn).sum() > 0 and (~mo & mn).sum() > 0, "zones at rest at the old, at both, at the new time"
    ratio = c.unew[0] / c.uold[0]
    assert (ratio > 9.9).sum() > 0 and (ratio < 0.101).sum() > 0, "the density changes by a factor of ten both ways"
    if c.const:
        for g in (c.gold, c.gnew):
            assert all(np.all(g[n] == c.vec[n]) for n in range(3))
    else:
        assert not np.array_equal(c.gold, c.gnew) and np.unique(c.gold[0]).size > c.gold[0].size // 2


@pytest.mark.parametrize("c", V.case_ids("grav"))
def test_gravity_source_restatement(c):
    c = V.gravity_case(c)
    gravity_branches(c)
    dx = [c.geom.dx[d] for d in range(3)]
    old = R.old_gravity_source(c.uold, c.box, c.gold, c.gbox, c.lo, c.hi, c.gtype, c.dt)
    new = R.new_gravity_source(c.uold, c.box, c.unew, c.box, c.M, c.fb, c.gold, c.gnew, c.gbox, c.lo, c.hi, c.gtype, c.dt, dx)
    for n in (1, 2, 3, 4):                      # each momentum source and the energy source, old and new, is not all zero
        assert np.abs(c.want_old[n]).max() > 0.0 and np.abs(c.want_new[n]).max() > 0.0, (c.P, n)
    assert V.same(old, c.want_old), "%s old: %d values differ" % (c.P, V.differing(old, c.want_old))
    assert V.same(new, c.want_new), "%s new: %d values differ" % (c.P, V.differing(new, c.want_new))
    count(c.want_old.size + c.want_new.size, c.want_old.size + c.want_new.size, 0, c.P + " (numpy)")


@pytest.mark.parametrize("c", [c for c in V.case_ids("grav") if V.gravity_case(c).const])
def test_gravity_source_oracle_with_one_vector(c):
    import ctypes as C
    c = V.gravity_case(c)
    L = O.lib()
    shp = (7,) + c.uold.shape[1:]
    uold, unew = np.ascontiguousarray(c.uold), np.ascontiguousarray(c.unew)
    M = [np.ascontiguousarray(m) for m in c.M]
    g = (C.c_double * 3)(*c.vec)
    dx = (C.c_double * 3)(*[c.geom.dx[d] for d in range(3)])
    old, new = np.zeros(shp), np.zeros(shp)
    L.ora_old_gravity_source(O.i3(c.lo), O.i3(c.hi), O.a4(uold, c.lo, c.hi), O.a4(old, c.lo, c.hi), C.byref(g), c.gtype, c.dt)
    mf = (O.A4 * 3)()
    for d in range(3):
        mf[d] = O.a4(M[d], c.fb[d][0], c.fb[d][1])
    L.ora_new_gravity_source(O.i3(c.lo), O.i3(c.hi), O.a4(uold, c.lo, c.hi), O.a4(unew, c.lo, c.hi), O.a4(new, c.lo, c.hi), mf,
                             C.byref(g), c.gtype, c.dt, C.byref(dx))
    assert V.same(old, c.want_old), "%s old: %d values differ" % (c.P, V.differing(old, c.want_old))
    assert V.same(new, c.want_new), "%s new: %d values differ" % (c.P, V.differing(new, c.want_new))
    count(old.size + new.size, old.size + new.size, 0, c.P + " (oracle)")


# ---- point mass ------------------------------------------------------------------------------------------------------------------
def test_pointmass_cases_cover_the_branches():
    cases = [V.pointmass_case(c) for c in V.case_ids("pm")]
    signs = set(np.sign(c.want_delta) for c in cases)
    assert signs == {1.0, -1.0, 0.0}
    corner = inside = cut = whole = several = cancel = mixed = missed = octants = 0
    for c in cases:
        frac = [(c.center[d] - c.geom.problo[d]) / c.geom.dx[d] for d in range(3)]
        at_corner = all(abs(f - round(f)) < 1e-6 for f in frac)
        corner, inside = corner + at_corner, inside + (not at_corner)
        cb = PR.cube(c.center, c.geom)
        n = sum(int(np.prod([h - l + 1 for l, h in zip(*PR.clip(cb, lo, hi))])) for lo, hi in c.boxes if PR.clip(cb, lo, hi))
        cut, whole = cut + (n < 64), whole + (n == 64)
        several += len(c.boxes) > 1 and sum(PR.clip(cb, lo, hi) is not None for lo, hi in c.boxes) > 1
        cancel += c.want_delta == 0.0 and np.any(c.want_parts != 0.0)
        mixed += c.want_delta > 0.0 and np.any(c.want_parts < 0.0)
        assert any(lo[d] < 0 for lo, hi in c.boxes for d in range(3))
        # boxes that miss the cube (the `slabs` cut of tests/test_pointmass_gpu.py): part 0, S_new as it was
        miss = [b for b, (lo, hi) in enumerate(c.boxes) if PR.clip(cb, lo, hi) is None]
        hit = [b for b in range(len(c.boxes)) if b not in miss]
        for b in miss:
            assert c.want_parts[b] == 0.0 and np.array_equal(c.want_snew[b], c.snew[b]) and not np.array_equal(c.snew[b], c.sold[b])
        missed += len(miss) >= 2 and len(hit) >= 2 and c.want_delta > 0.0
        # the cube cut in all three directions at once (the `eight` cut): eight boxes with 8 cube zones each
        octants += len(c.boxes) == 8 and all(int(np.prod([h - l + 1 for l, h in zip(*PR.clip(cb, lo, hi))])) == 8 for lo, hi in c.boxes) \
            and c.want_delta > 0.0
    assert min(corner, inside, cut, whole, several, cancel, mixed, missed, octants) >= 1, \
        (corner, inside, cut, whole, several, cancel, mixed, missed, octants)


@pytest.mark.parametrize("c", V.case_ids("pm"))
def test_pointmass_restatement(c):
    c = V.pointmass_case(c)
    new = [s.copy() for s in c.snew]
    boxes = [(lo, hi, so, (lo, hi), sn, (lo, hi)) for (lo, hi), so, sn in zip(c.boxes, c.sold, new)]
    parts = np.array(PR.delta_parts(boxes, c.geom, c.center))
    d = PR.delta(boxes, c.geom, c.center)
    assert np.array_equal(parts, c.want_parts), (c.P, parts, c.want_parts)
    assert d == c.want_delta, (c.P, d, c.want_delta)
    m = PR.apply(boxes, c.geom, c.center, d, c.mass)
    assert m == c.want_mass and (m > c.mass) == (d > 0.0)
    for b, (sn, w, before) in enumerate(zip(new, c.want_snew, c.snew)):
        assert V.same(sn, w), "%s box %d: %d values differ" % (c.P, b, V.differing(sn, w))
    changed = any(not np.array_equal(w, s) for w, s in zip(c.want_snew, c.snew))
    assert changed == (c.want_delta > 0.0)
    n = sum(w.size for w in c.want_snew) + c.want_parts.size + 2
    count(n, n, 0, c.P)

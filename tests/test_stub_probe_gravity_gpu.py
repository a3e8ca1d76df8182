"""The device entry points of monopole gravity, the point mass and the multipole boundary against
tests/golden/stub_probe/gravity_vectors.npz: outputs of the reference's own Gravity::install_level, compute_radial_mass,
make_radial_gravity, interpolate_monopole_grav, add_pointmass_to_gravity, init_multipole_grav and fill_multipole_BCs, compiled
unmodified against stand-in headers (tools/stub_probe/probe_gravity.cpp; STUB-COMPILED, NOT oracle/_ref), replayed through
castro_amd_radial_mass_mf / _mf_ex, castro_amd_radial_combine, castro_amd_radial_gravity, castro_amd_monopole_grav_fab,
castro_amd_add_pointmass_fab / _mf, castro_amd_multipole_moments_mf and castro_amd_multipole_phi_bc_fab in both numerics builds.
The comparison is with the RECORDED outputs; the restatements only supply the bounds.  tests/test_stub_probe_gravity.py replays
the same cases on the CPU and asserts that the fixture holds every branch.  Only the fixture is read.

Tolerances -- none of them new.  `exact`: bit for bit wherever the CPU replay asks bit equality of an order-free quantity (the
combined profile and radial_grav from the recorded arrays, the interpolated gravity, the point-mass sums, the kept sentinels, the
r < 1e-12 zero, the untouched interior; the bin masses and volumes of the dyadic cases, whose sums are exact in any order).
`contract`: those within 1e-10 of the largest magnitude (_close of tests/test_monopole_gpu.py; the point mass by its own test's
1e-10 (|before| + |term|)).  Both builds: a bin mass of full-mantissa densities within monopole_ref.mass_bounds of the recording
(two orders of the same terms), a bin volume within count * 2**-53 * volume of it (the device forms count * vol_frac, the
reference adds vol_frac count times), the moments and the boundary potential within the allowances of tests/poisson_ref.py.

Every FAB a call may write sits between two runs of a canary value in one allocation."""
import math

import numpy as np
import pytest
import torch

from tests import monopole_ref as R
from tests import pointmass_ref as PR
from tests import poisson_ref as Q
from tests import stub_probe_gravity as V
from tests.test_monopole_gpu import _close
from tests.test_stub_probe_gravity import _ratio, level_rho, mp_moments, rg_ref, rm_ref, vol_bound, want_q
from tests.test_stub_probe_sources_gpu import Guarded, _fab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["exact", "contract"])
def hydro(request):
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=request.param)
    yield h
    h.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _state(rho, bx):
    """(tensor, box): an 8-component state FAB with two NaN ghost zones around the valid zones; only the density is read"""
    U = np.full((8,) + rho.shape, 0.5)
    U[0] = rho
    F, fbox = _fab(U, bx[0], bx[1], 2, np.nan)
    return _t(F), fbox


def _mask(m):
    return None if m is None else _t(np.ascontiguousarray(m, dtype=np.uint8))


def _check_bins(h, got, ref, want_mass, want_vol, n1d, what, dyadic):
    mass, vol = got[:n1d], got[n1d:]
    assert np.array_equal(vol, ref["vol"]), what + ": count * vol_frac of the counted sub-zones"
    eb, em = np.abs(vol - want_vol), np.abs(mass - want_mass)
    print("%s (%s): mass deviation / mass_bounds %.3g, volume deviation / bound %.3g"
          % (what, h.numerics, _ratio(em, R.mass_bounds(ref)), _ratio(eb, vol_bound(ref))))
    assert np.all(eb <= vol_bound(ref)) and np.all(em <= R.mass_bounds(ref)), what
    if dyadic:
        assert V.same(mass, want_mass) and V.same(vol, want_vol), what + ": dyadic inputs, every sum exact in any order"


def _is_dyadic(dx):
    return all(math.frexp(x)[0] in (0.5, 0.625, 0.75, 0.875) for x in dx)


@pytest.mark.parametrize("i", V.case_ids("rm"))
def test_radial_mass_mf(hydro, i):
    c, ref = rm_ref(i)
    keep = [_state(rho, bx) for rho, bx in zip(c.rho, c.bx)]
    table = hydro.make_diag_boxes([(bx[0], bx[1], s, None) for bx, s in zip(c.bx, keep)])
    out = Guarded(np.full(2 * c.n1d, np.nan))
    hydro.radial_mass_mf(table, c.geom, c.mono, out.t)
    torch.cuda.synchronize()
    _check_bins(hydro, out.numpy(), ref, c.want_mass, c.want_vol, c.n1d, c.P, _is_dyadic(c.dx))


@pytest.mark.parametrize("i", V.case_ids("rg"))
def test_radial_gravity_chain(hydro, i):
    c, refs = rg_ref(i)
    own = []
    for l in range(c.level + 1):
        branch, boxes = level_rho(c, l)
        n1d = c.want_n1d[l]
        out = Guarded(np.full(2 * n1d, np.nan))
        masks = [_mask(b[2]) for b in boxes]
        if branch == "mix":
            _, oa, al = V.time_branch(c.time, *c.times[l])
            so = [_state(r, bx) for r, bx in zip(c.rho_old[l], c.boxes[l])]
            sn = [_state(r, bx) for r, bx in zip(c.rho_new[l], c.boxes[l])]
            table = hydro.make_radial_boxes([(bx[0], bx[1], o, n, m) for bx, o, n, m in zip(c.boxes[l], so, sn, masks)])
            hydro.radial_mass_mf_ex(table, oa, al, c.geoms[l], c.monos[l], out.t)
        else:
            st = [_state(b[0], bx) for b, bx in zip(boxes, c.boxes[l])]
            table = hydro.make_diag_boxes([(bx[0], bx[1], s, m) for bx, s, m in zip(c.boxes[l], st, masks)])
            hydro.radial_mass_mf(table, c.geoms[l], c.monos[l], out.t)
        torch.cuda.synchronize()
        got = out.numpy()
        _check_bins(hydro, got, refs[l], c.want_mass[l], c.want_vol[l], n1d, "%slevel %d (%s)" % (c.P, l, branch), _is_dyadic(c.dx))
        own.append(_t(got))
    # the combination and the integration from the RECORDED arrays: a fixed order
    n = c.want_n1d[c.level]
    rec = [_t(np.concatenate([c.want_mass[l], c.want_vol[l]])) for l in range(c.level + 1)]
    grav = {}
    for name, arrays in (("recorded", rec), ("own", own)):
        summed, rg = Guarded(np.full(2 * n, np.nan)), Guarded(np.full(n, np.nan))
        hydro.radial_combine(c.level, arrays, c.want_n1d[:c.level + 1], summed.t)
        hydro.radial_gravity(c.monos[c.level], c.geoms[c.level], summed.t, rg.t)
        torch.cuda.synchronize()
        summed.numpy()
        grav[name] = rg.numpy()
    _close(hydro, grav["recorded"], c.want_grav, c.P + "radial_grav from the recorded radial_mass / radial_vol")
    dev = np.abs(grav["own"] - c.want_grav).max() / np.abs(c.want_grav).max()
    print("%sradial_grav of the device's own bins (%s): %.3g of the largest magnitude from the recording" % (c.P, hydro.numerics, dev))
    assert dev <= 1e-10


@pytest.mark.parametrize("i", V.case_ids("ig"))
def test_monopole_grav(hydro, i):
    c = V.interpolate_case(i)
    rg = _t(c.rg)
    for b, gbox in enumerate(c.gbox):
        g = Guarded(np.full(c.want[b].shape, c.fill))
        hydro.monopole_grav(rg, c.mono, c.geom, g.t, gbox)
        torch.cuda.synchronize()
        got, want = g.numpy(), c.want[b]
        kept = want == c.fill
        assert kept.any() and (~kept).any()
        assert np.array_equal(got[kept], want[kept]), "%sa zone beyond the last bin keeps what it held" % c.P
        _close(hydro, got[~kept], want[~kept], "%sbox %d" % (c.P, b))


@pytest.mark.parametrize("i", V.case_ids("pg"))
def test_add_pointmass(hydro, i):
    from castro_amd import _lib
    c = V.pointmass_case(i)
    pm = _lib.make_pointmass(c.center, _lib.GCONST)
    mass = torch.tensor([c.mass, -1.0], dtype=torch.float64, device="cuda")

    def check(got, b, what):
        want = c.want_grav[b].reshape(got.shape)
        if hydro.numerics == "exact":
            assert V.same(got, want), "%s: %d entries differ" % (what, int((got != want).sum()))
        else:
            term = PR.pointmass_term(c.gbox[b], c.geom, c.center, _lib.GCONST, c.mass)
            ratio = (np.abs(got - want) / (1e-10 * (np.abs(c.grav[b]) + np.abs(term)))).max()
            print("%s (contract): largest deviation / bound = %.3g" % (what, ratio))
            assert ratio <= 1.0

    mf = []
    for b, gbox in enumerate(c.gbox):
        g = Guarded(c.grav[b])
        hydro.add_pointmass(g.t, gbox, pm, c.geom, mass)
        torch.cuda.synchronize()
        check(g.numpy(), b, "%sadd_pointmass box %d" % (c.P, b))
        mf.append(Guarded(c.grav[b]))
    hydro.add_pointmass_mf(hydro.make_grav_fabs([(g.t, gbox) for g, gbox in zip(mf, c.gbox)]), pm, c.geom, mass)
    torch.cuda.synchronize()
    for b, g in enumerate(mf):
        check(g.numpy(), b, "%sadd_pointmass_mf box %d" % (c.P, b))


@pytest.mark.parametrize("i", V.case_ids("mp"))
def test_multipole_moments_and_phi_bc(hydro, i):
    from castro_amd import _lib
    c = V.multipole_case(i)
    mp = _lib.make_multipole(c.geoms[0], c.center, c.lnum)
    assert mp.rmax == float(c.want_rmax[0])
    n1 = c.lnum + 1
    _, bound = mp_moments(c)
    want = want_q(c)
    q = np.zeros(3 * n1 * n1)
    for l in range(c.nlev):
        st = [_state(r, bx) for r, bx in zip(c.rho[l], c.boxes[l])]
        masks = [_mask(None if m is None else (m != 0.0)) for m in c.mask[l]]
        table = hydro.make_diag_boxes([(bx[0], bx[1], s, m) for bx, s, m in zip(c.boxes[l], st, masks)])
        out = Guarded(np.full(3 * n1 * n1, np.nan))
        hydro.multipole_moments_mf(table, c.geoms[l], mp, out.t)
        torch.cuda.synchronize()
        q = q + out.numpy()
    err = np.abs(q - want)
    print("%smoments (%s): worst deviation / allowance %.3g" % (c.P, hydro.numerics, _ratio(err, bound)))
    assert np.all(err <= bound)
    # the boundary potential from the recorded moments
    phi = Guarded(c.phi[None])
    hydro.multipole_phi_bc(phi.t, c.pbox, c.geoms[0], mp, _t(want))
    torch.cuda.synchronize()
    got = phi.numpy()[0]
    ref = c.phi.copy()
    outside, allow = Q.phi_bc(want, c.geoms[0], mp, ref, c.pbox)
    assert V.same(got[~outside], c.want_phi[~outside]), "the interior is untouched"
    err = np.abs(got - c.want_phi)
    print("%sphi_bc (%s): worst deviation / allowance %.3g" % (c.P, hydro.numerics, _ratio(err[outside], allow[outside])))
    assert np.all(err <= allow)
    zero = c.want_phi == 0.0
    assert V.same(got[zero], c.want_phi[zero]), "the r < 1e-12 zone holds +0.0"

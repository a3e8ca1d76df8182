"""The device source terms against tests/golden/stub_probe/source_vectors.npz: outputs of the reference's own
Castro::apply_sponge / construct_new_sponge_source, construct_old/new_gravity_source (grav_source_type 1-4) and
Castro::pointmass_update, compiled unmodified against stand-in headers (tools/stub_probe/probe_sources.cpp; STUB-COMPILED, NOT
oracle/_ref), replayed through castro_amd_new_sponge_source_fab, castro_amd_old/new_gravity_source_fab and _gfab,
castro_amd_pointmass_delta_mf / _apply_mf and, where a one-pass form exists, castro_amd_sources_mf / _mf_g / _mf_opts, stage 0
and stage 1, in both numerics builds.  tests/test_stub_probe_sources.py replays the same cases on the CPU restatements and
asserts that the cases reach the branches.  Only the fixture is read.

Tolerances -- none of them new.  `exact`: every recorded value bit for bit, except a sponge zone whose factor went through the
ramp's cos, where the device cos may differ from libm's: the bound of
tests/test_sponge_gpu.py::test_zone_function_against_the_restatement (sponge_ref.cos_bound through its _scales).  `contract`:
the sponge by that test's 1e-10 of the same scales; the gravity sources by _close of tests/test_monopole_gpu.py (1e-10 of a
component's largest magnitude); the point mass as tests/test_pointmass_gpu.py::test_delta_and_apply has it for both builds: the
mass change within 64 * 2^-52 * sum |vol drho|, the restore and the sign test bit for bit.

The device refuses sponge_timescale <= 0 as the reference's start-up check does (Castro.cpp:475-488), so the two alpha = 0
cases, which only Castro::apply_sponge itself accepts, are replayed as that refusal: the source FAB keeps what it held.

Every FAB a call may write sits between two runs of a canary value in one allocation, and the ghost zones of a single-FAB call
hold the canary too: all of it must still be there afterwards."""
import numpy as np
import pytest
import torch

from tests import monopole_ref as R
from tests import pointmass_ref as PR
from tests import sponge_ref as S
from tests import stub_probe_sources as V
from tests.test_monopole_gpu import _close
from tests.test_sponge_gpu import _scales

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CANARY, PAD = 7.25, 64


@pytest.fixture(scope="module", params=["exact", "contract"])
def hydro(request):
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=request.param)
    yield h
    h.close()


class Guarded:
    """a FAB tensor in the middle of one allocation, PAD canary doubles on either side"""

    def __init__(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.buf = torch.full((a.size + 2 * PAD,), CANARY, dtype=torch.float64, device="cuda")
        self.t = self.buf[PAD:PAD + a.size].view(a.shape)
        self.t.copy_(torch.from_numpy(a))
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + 8 * PAD

    def numpy(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:PAD] == CANARY) and np.all(b[-PAD:] == CANARY), "a write outside the FAB"
        return b[PAD:-PAD].reshape(tuple(self.t.shape)).copy()


def _fab(valid, lo, hi, ng, fill):
    """(array, box): `valid` on [lo, hi] inside a FAB with ng ghost zones that hold `fill`"""
    n = valid.shape[1:]
    F = np.full((valid.shape[0],) + tuple(x + 2 * ng for x in n), fill)
    F[(slice(None),) + tuple(slice(ng, ng + x) for x in n)] = valid
    return F, (tuple(x - ng for x in lo), tuple(x + ng for x in hi))


def _split(got, box, lo, hi):
    """(the zones of [lo, hi], everything else) of a FAB array on `box`"""
    v = (slice(None),) + R._sl(box, lo, hi)
    ghost = np.ones(got.shape, dtype=bool)
    ghost[v] = False
    return got[v], got[ghost]


def _params(gamma=1.4):
    from castro_amd import _lib
    P = _lib.default_params()
    assert P.eos_gamma == gamma and P.abar == 1.0, "the gamma-law gas of the recording (stub/eos.H)"
    return P


# ---- sponge ----------------------------------------------------------------------------------------------------------------------
def _check_sponge(h, c, got, what):
    k = [S.UMX, S.UMY, S.UMZ, S.UEDEN]
    for n in (S.URHO, S.UEINT, S.UTEMP):
        assert np.all(got[n] == 0.0), what
    info = {}
    from types import SimpleNamespace
    S.apply_sponge(c.U, c.box, c.lo, c.hi, c.sponge, c.geom, SimpleNamespace(eos_gamma=c.eos_gamma, abar=1.0), c.dt, info)
    cosm = info["cos"]                         # which zones evaluate a ramp: a property of the inputs
    g, w = got[k], c.want[k]
    d = np.abs(g - w)
    scale = _scales(c.U, c.want, S.cos_bound(c.U, c.box, c.lo, c.hi, c.sponge, c.want, c.dt))
    assert c.step == (not cosm.any()) and (~cosm).any()
    if h.numerics == "exact":
        flat = ~cosm
        assert V.same(g[:, flat], w[:, flat]), "%s: %d values outside every ramp differ" % (what, V.differing(g[:, flat], w[:, flat]))
        # a zone at rest with no target velocity has bound 0 and source 0: the bound is applied value by value, not as a ratio
        ratio = (d[:, cosm] / np.where(scale[:, cosm] > 0.0, scale[:, cosm], 1.0)).max() if cosm.any() else 0.0
        print("%s (exact): %d values bit for bit, %d ramp values, largest |device - reference| / bound = %.3g, %d of them bit-equal"
              % (what, int(4 * flat.sum()) + 3 * flat.size, int(4 * cosm.sum()), ratio, int((d[:, cosm] == 0).sum())))
        assert np.all(d[:, cosm] <= scale[:, cosm]), ratio
    else:
        ref = scale / (8.0 * EPS)
        ratio = (d / np.where(ref > 0.0, ref, 1.0)).max()
        print("%s (contract): %d values, largest deviation / scale = %.3g" % (what, w.size, ratio))
        assert np.all(d <= 1e-10 * ref), ratio


@pytest.mark.parametrize("c", V.case_ids("sponge"))
def test_sponge(hydro, c):
    c = V.sponge_case(c)
    P = _params(c.eos_gamma)
    U, ub = _fab(c.U, c.lo, c.hi, 2, np.nan)
    base, sb = _fab(np.zeros((7,) + c.U.shape[1:]), c.lo, c.hi, 1, CANARY)
    Ud = Guarded(U)
    # the single-FAB entry point
    src = Guarded(base)
    if not c.timescale > 0.0:
        with pytest.raises(RuntimeError):
            hydro.new_sponge_source(Ud.t, ub, src.t, sb, c.lo, c.hi, c.sponge, c.geom, P, c.dt)
        boxes = hydro.make_source_boxes([(c.lo, c.hi, (Ud.t, ub), (Ud.t, ub), (src.t, sb), [None] * 3, [(c.lo, c.hi)] * 3)])
        with pytest.raises(RuntimeError):
            hydro.sources_mf(1, boxes, None, 4, None, c.geom, P, c.dt, ntimes=0, sponge=c.sponge)
        torch.cuda.synchronize()
        assert np.array_equal(src.numpy(), base) and np.all(c.want == 0.0), "refused, nothing written; the reference adds zeros"
        return
    hydro.new_sponge_source(Ud.t, ub, src.t, sb, c.lo, c.hi, c.sponge, c.geom, P, c.dt)
    torch.cuda.synchronize()
    got, ghost = _split(src.numpy(), sb, c.lo, c.hi)
    assert np.all(ghost == CANARY), "only [lo, hi] is written"
    _check_sponge(hydro, c, got, c.P + " new_sponge_source_fab")
    assert V.same(Ud.numpy(), U), "the state is read only"
    # the one-pass form: stage 1 adds the sponge, stage 0 takes one and adds nothing
    for stage in (1, 0):
        So, Sn, src = Guarded(U), Guarded(U), Guarded(np.full(base.shape, 3.0))
        boxes = hydro.make_source_boxes([(c.lo, c.hi, (So.t, ub), (Sn.t, ub), (src.t, sb), [None] * 3, [(c.lo, c.hi)] * 3)])
        hydro.sources_mf(stage, boxes, None, 4, None, c.geom, P, c.dt, ntimes=0, sponge=c.sponge)
        torch.cuda.synchronize()
        got, ghost = _split(src.numpy(), sb, c.lo, c.hi)
        assert np.all(ghost == 0.0), "the one-pass call zeroes the ghost zones of the source FAB"
        if stage == 1:
            _check_sponge(hydro, c, got, c.P + " sources_mf_opts stage 1")
        else:
            assert np.all(got == 0.0)
        new, nghost = _split(Sn.numpy(), ub, c.lo, c.hi)
        assert np.all(np.isnan(nghost)) and V.same(So.numpy(), U)
        assert np.array_equal(new[[S.URHO, S.UEINT, S.UTEMP, S.UFS]], c.U[[S.URHO, S.UEINT, S.UTEMP, S.UFS]])
        upd = c.U[1:5] + c.dt * got[1:5]
        assert np.abs(new[1:5] - upd).max() <= 4.0 * EPS * np.abs(upd).max()


# ---- gravity sources -------------------------------------------------------------------------------------------------------------
def _check_gravity(h, got, want, what):
    n = 0
    for k in range(7):
        if np.abs(want[k]).max() == 0.0:
            assert np.all(got[k] == 0.0), (what, k)
        else:
            _close(h, got[k], want[k], "%s, component %d" % (what, k))
        n += want[k].size
    return n


@pytest.mark.parametrize("c", V.case_ids("grav"))
def test_gravity_sources(hydro, c):
    c = V.gravity_case(c)
    P = _params()
    UO, ub = _fab(c.uold, c.lo, c.hi, 2, np.nan)
    UN, _ = _fab(c.unew, c.lo, c.hi, 2, np.nan)
    base, sb = _fab(np.zeros((7,) + c.uold.shape[1:]), c.lo, c.hi, 1, CANARY)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    uo, un, M, go, gn = t(UO), t(UN), [t(m) for m in c.M], t(c.gold), t(c.gnew)
    n = 0
    # the single-FAB entry points: the vector form where the recording held one vector, the FAB form always
    forms = (["vector"] if c.const else []) + ["fab"]
    for form in forms:
        so, sn = Guarded(base), Guarded(base)
        if form == "vector":
            hydro.old_gravity_source(uo, ub, so.t, sb, c.lo, c.hi, c.vec, c.gtype, c.dt)
            hydro.new_gravity_source(uo, ub, un, ub, sn.t, sb, M, c.fb, c.lo, c.hi, c.vec, c.gtype, c.dt, c.geom)
        else:
            hydro.old_gravity_source_gfab(uo, ub, so.t, sb, c.lo, c.hi, go, c.gbox, c.gtype, c.dt)
            hydro.new_gravity_source_gfab(uo, ub, un, ub, sn.t, sb, M, c.fb, c.lo, c.hi, go, gn, c.gbox, c.gtype, c.dt, c.geom)
        torch.cuda.synchronize()
        for s, want, when in ((so, c.want_old, "old"), (sn, c.want_new, "new")):
            got, ghost = _split(s.numpy(), sb, c.lo, c.hi)
            assert np.all(ghost == CANARY), "only [lo, hi] is written"
            n += _check_gravity(hydro, got, want, "%s %s source, %s form, type %d" % (c.P, when, form, c.gtype))
    # the one-pass forms, stage 0 (old-time source, S_new = S_old + dt source) and stage 1 (new-time source, S_new += dt source)
    for form in forms:
        for stage, want in ((0, c.want_old), (1, c.want_new)):
            So, Sn, src = Guarded(UO), Guarded(UN), Guarded(np.full(base.shape, 3.0))
            boxes = hydro.make_source_boxes([(c.lo, c.hi, (So.t, ub), (Sn.t, ub), (src.t, sb), M, c.fb)])
            if form == "vector":
                hydro.sources_mf(stage, boxes, c.vec, c.gtype, None, c.geom, P, c.dt, ntimes=0)
            else:
                hydro.sources_mf_g(stage, boxes, hydro.make_grav_fabs([(go, c.gbox)]), hydro.make_grav_fabs([(gn, c.gbox)]), c.gtype, None,
                                   c.geom, P, c.dt, ntimes=0)
            torch.cuda.synchronize()
            got, ghost = _split(src.numpy(), sb, c.lo, c.hi)
            assert np.all(ghost == 0.0), "the one-pass call zeroes the ghost zones of the source FAB"
            n += _check_gravity(hydro, got, want, "%s one pass, stage %d, %s form, type %d" % (c.P, stage, form, c.gtype))
            new, nghost = _split(Sn.numpy(), ub, c.lo, c.hi)
            assert np.all(np.isnan(nghost)) and V.same(So.numpy(), UO)
            start = c.uold if stage == 0 else c.unew
            upd = start[1:5] + c.dt * got[1:5]
            assert np.abs(new[1:5] - upd).max() <= 4.0 * EPS * np.abs(upd).max()
            assert np.array_equal(new[[0, 5, 6, 7]], start[[0, 5, 6, 7]])
    assert np.array_equal(go.cpu().numpy(), c.gold) and np.array_equal(gn.cpu().numpy(), c.gnew)
    print("%s (%s): %d recorded values compared, %s" % (c.P, hydro.numerics, n, "bit for bit" if hydro.numerics == "exact"
                                                        else "within 1e-10 of a component's largest magnitude"))


# ---- point mass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", V.case_ids("pm"))
def test_pointmass(hydro, c):
    from castro_amd import _lib
    c = V.pointmass_case(c)
    pm = _lib.make_pointmass(c.center, 6.67428e-8)
    fo = [_fab(s, lo, hi, 2, CANARY) for s, (lo, hi) in zip(c.sold, c.boxes)]
    fn = [_fab(s, lo, hi, 2, CANARY) for s, (lo, hi) in zip(c.snew, c.boxes)]
    do, dn = [Guarded(f[0]) for f in fo], [Guarded(f[0]) for f in fn]
    tab = hydro.make_pointmass_boxes([(lo, hi, (a.t, o[1]), (b.t, n[1])) for (lo, hi), a, b, o, n in zip(c.boxes, do, dn, fo, fn)])
    buf = Guarded(np.array([c.mass, np.nan]))
    hydro.pointmass_delta_mf(tab, pm, c.geom, buf.t[1:])
    torch.cuda.synchronize()
    m0, got = buf.numpy()
    assert m0 == c.mass
    for d, f in zip(dn, fn):
        assert V.same(d.numpy(), f[0]), "the sum writes no state"
    terms = PR.delta_terms([(lo, hi, so, (lo, hi), sn, (lo, hi)) for (lo, hi), so, sn in zip(c.boxes, c.sold, c.snew)], c.geom, c.center)
    bound = 64 * EPS * np.abs(terms).sum()
    print("%s (%s): mass change %.17g, recorded %.17g, |difference| / (64 eps sum |terms|) = %.3g"
          % (c.P, hydro.numerics, got, c.want_delta, abs(got - c.want_delta) / bound if bound else 0.0))
    if hydro.numerics == "exact":
        assert got == c.want_delta
    else:
        assert abs(got - c.want_delta) <= bound
    assert np.sign(got) == np.sign(c.want_delta)
    hydro.pointmass_apply_mf(tab, pm, c.geom, buf.t[1:], buf.t[:1])
    torch.cuda.synchronize()
    m1, d1 = buf.numpy()
    assert d1 == got and m1 == (c.mass + got if got > 0.0 else c.mass)
    if hydro.numerics == "exact":
        assert m1 == c.want_mass
    n = 2
    for d, o, f, (lo, hi), w in zip(dn, do, fn, c.boxes, c.want_snew):
        new, ghost = _split(d.numpy(), f[1], lo, hi)
        assert np.all(ghost == CANARY), "only zones of the box are written"
        assert V.same(new, w), "%s: %d values of S_new differ" % (c.P, V.differing(new, w))
        n += w.size
    for o, f in zip(do, fo):
        assert V.same(o.numpy(), f[0]), "S_old is read only"
    print("%s (%s): %d recorded values compared, the restore bit for bit" % (c.P, hydro.numerics, n))

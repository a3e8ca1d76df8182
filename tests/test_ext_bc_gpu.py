"""castro_amd_ext_bc_fill_fab (k_ambient_fill, k_hse_fill) on the device.

Replay: every case of tests/golden/stub_probe/bc_vectors.npz -- the reference's own ambient_fill and hse_fill, stub-compiled
(tests/ext_bc_cases.py) -- in both numerics builds.  `exact`: every value bit for bit; the fill uses + - * / min max abs only,
with IEEE division and no contraction in that build.  `contract`: the project's rtol 1e-10 as smoke() has it (_close).  The FAB sits
between two runs of a canary value, which must still be there afterwards.

The counter of unconverged columns stays 0 on the converging cases and counts the columns of the case whose temperature
hse_interp_temp extrapolates below zero (the reference's arithmetic stays finite there: every update is clamped to 10 %; recorded
with the reference's GPU form of hse_fill.cpp, which does not abort) -- the number the restatement counts on the CPU.

Drivers: Castro(ext_bc=...) and CastroAmr(ext_bc=...) on the device against the CPU drivers of tests/test_ext_bc_cpu.py, whose
backend applies the numpy restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ext_bc_cases as X
from tests import ext_bc_ref as R

pytestmark = pytest.mark.gpu

CANARY, PAD = 7.25, 64
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2


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

    def numpy(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:PAD] == CANARY) and np.all(b[-PAD:] == CANARY), "a write outside the FAB"
        return b[PAD:-PAD].reshape(tuple(self.t.shape)).copy()


def _close(h, got, want, what, bits=True):
    """`exact`: the same bits.  `contract`: rtol 1e-10 as smoke() has it -- every scalar component against its own largest
    magnitude, the three momenta against the largest magnitude of any of them (one vector, one scale: a component that vanishes
    by symmetry holds rounding noise only)"""
    if h.numerics == "exact":
        same = X.bits_equal(got, want) if bits else np.array_equal(got, want)           # the drivers: as values, like the other driver tests
        assert same, "%s: %d values differ" % (what, int((got.view(np.int64) != want.view(np.int64)).sum()))
        return
    mom = max(np.abs(want[n]).max() for n in (1, 2, 3))
    for n in range(want.shape[0]):
        d, m = np.abs(got[n] - want[n]).max(), mom if n in (1, 2, 3) else np.abs(want[n]).max()
        print("%s component %d (contract): max deviation %.3g of %.3g" % (what, n, d, m))
        assert d <= 1e-10 * m, (what, n, d, m)


def _raw(h, U, box, geom, params, ext, counter=None):
    from castro_amd import _lib as L
    return h.lib.castro_amd_ext_bc_fill_fab(h.h, C.byref(L.fab_of(U, *box)), C.byref(geom), C.byref(params), C.byref(ext),
                                            None if counter is None else counter.data_ptr(), None)


@pytest.mark.parametrize("c", range(X.ncases()))
def test_replay_of_the_reference(hydro, c):
    box, geom, params, ext, U_in, U_out, silent = X.case(c)
    G = Guarded(U_in)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    hydro.ext_bc_fill(G.t, box, geom, params, ext, unconverged=counter)
    got = G.numpy()
    _close(hydro, got, U_out, "bc%d" % c)
    inside = (slice(None),) + tuple(slice(max(geom.domlo[d], box[0][d]) - box[0][d], min(geom.domhi[d], box[1][d]) - box[0][d] + 1)
                                    for d in (2, 1, 0))
    assert X.bits_equal(got[inside], U_in[inside]), "a zone of the domain was written"
    want = R.ext_bc_fill(U_in.copy(), box, geom, params, ext)
    assert (want > 0) == silent
    if hydro.numerics == "exact" or not silent:
        assert int(counter.item()) == want
    else:
        print("bc%d (contract): %d unconverged columns, restatement %d" % (c, int(counter.item()), want))
        assert int(counter.item()) > 0
    # without a counter the same zones
    G2 = Guarded(U_in)
    hydro.ext_bc_fill(G2.t, box, geom, params, ext)
    assert X.bits_equal(G2.numpy(), got)


def test_refusals_return_their_codes(hydro):
    from castro_amd import _lib as L
    box, geom, params, ext, U_in, _, _ = X.case(4)              # z low
    INFLOW = 1

    def run(geom=geom, ext=ext, U=U_in, box=box):
        G = Guarded(U)
        rc = _raw(hydro, G.t, box, geom, params, ext)
        return rc, X.bits_equal(G.numpy(), U)

    assert run()[0] == OK
    g = L.Geom.from_buffer_copy(geom)
    g.coord = 1
    assert run(geom=g) == (ERR_UNSUPPORTED, True)
    # +z HSE on an Inflow face
    g, e = L.Geom.from_buffer_copy(geom), L.ExtBc.from_buffer_copy(ext)
    g.lo_bc[2], g.hi_bc[2] = 2, INFLOW
    e.lo_type[2], e.hi_type[2] = -1, 1
    assert run(geom=g, ext=e) == (ERR_UNSUPPORTED, True)
    e.hi_type[2] = -1                   # an Inflow +z face without the type: nothing to refuse, nothing to do
    assert run(geom=g, ext=e) == (OK, True)
    # two Inflow faces that meet at an edge, whatever their types; opposite faces are fine
    for d in (0, 1):
        for side in (0, 1):
            g = L.Geom.from_buffer_copy(geom)
            (g.lo_bc if side == 0 else g.hi_bc)[d] = INFLOW
            assert run(geom=g) == (ERR_UNSUPPORTED, True), (d, side)
    g = L.Geom.from_buffer_copy(geom)
    g.hi_bc[2] = INFLOW
    assert run(geom=g)[0] == OK
    # hse_interp_temp with a domain of one zone in that direction
    g, e = L.Geom.from_buffer_copy(geom), L.ExtBc.from_buffer_copy(ext)
    g.domhi[2] = g.domlo[2]
    e.hse_interp_temp = 1
    assert run(geom=g, ext=e) == (ERR_ARG, True)
    # ... and with a FAB that holds one zone of the domain only: the extrapolation would read outside it
    e = L.ExtBc.from_buffer_copy(ext)
    e.hse_interp_temp = 1
    nz = geom.domlo[2] - box[0][2] + 1
    assert run(ext=e, U=U_in[:, :nz].copy(), box=(box[0], box[1][:2] + (geom.domlo[2],))) == (ERR_ARG, True)
    # the Python entry names the reason
    g = L.Geom.from_buffer_copy(geom)
    g.lo_bc[0] = INFLOW
    with pytest.raises(ValueError, match="corner"):
        hydro.ext_bc_fill(Guarded(U_in).t, box, g, params, ext)


def test_a_fab_that_is_not_the_state_is_left_alone(hydro):
    box, geom, params, ext, U_in, _, _ = X.case(4)
    G = Guarded(U_in[:7].copy())
    assert _raw(hydro, G.t, box, geom, params, ext) == OK           # Castro_bc_fill_nd.cpp:47-49
    assert X.bits_equal(G.numpy(), U_in[:7])


# ---- the drivers ------------------------------------------------------------------------------------------------------------------
def test_castro_with_a_hydrostatic_boundary_equals_the_cpu_driver(hydro, oracle):
    """the atmosphere of tests/test_ext_bc_cpu.py, 8 zones across (the problem is one-dimensional), 12 steps"""
    import castro_amd
    from castro_amd import _lib as L
    from tests.test_ext_bc_cpu import ATMOS, _atmosphere_run
    from tests.test_driver_cpu import _hse_atmosphere
    n = (8, 8, 32)
    ext = L.make_ext_bc(zl="hse")
    cpu, _ = _atmosphere_run(oracle, n, ext, 12)
    c = castro_amd.Castro(n, params=L.default_params(), hydro=hydro, ext_bc=ext, **ATMOS)
    c.set_state(_hse_atmosphere(n))
    for _ in range(12):
        c.step(1.0)
    if hydro.numerics == "exact":
        assert c.dt == cpu.dt and c.time == cpu.time
    _close(hydro, c.S_new().cpu().numpy(), cpu.S_new().numpy(), "Castro(ext_bc)", bits=False)
    assert not c.bc_in_hydro
    c.close()


def test_run_steps_with_an_ambient_boundary_replays_a_graph_and_equals_step_by_step(hydro):
    """a blast inside Outflow faces that carry an ambient state of half the density: the host-free batch (a captured pair of steps,
    replayed) against step(), bit for bit; the ambient fill is in both, and changes the answer"""
    import castro_amd
    from castro_amd import _lib as L
    n, nsteps = (16, 16, 16), 10
    ext = L.make_ext_bc(fill_ambient_bc=1, ambient_outflow_vel=1, ambient_density=0.5, ambient_energy=2.5e-5, ambient_temp=1.0)

    def make(e):
        c = castro_amd.Castro(n, params=L.default_params(), hydro=hydro, ext_bc=e, use_retry=False)
        c.initData("sedov", r_init=0.3, nsub=4)
        return c
    a, b, plain = make(ext), make(ext), make(None)
    assert a.host_free_ok()
    for _ in range(nsteps):
        a.step(1.0)
        plain.step(1.0)
    b.run_steps(nsteps, 1.0)
    assert getattr(b, "_graph_error", None) is None and len(b._graphs) > 0, "the batch was not replayed from a graph"
    assert b.nstep == a.nstep == nsteps and b.time == a.time
    Sa, Sb = a.S_new().cpu().numpy(), b.S_new().cpu().numpy()
    assert np.array_equal(Sa, Sb)
    assert not np.array_equal(Sa, plain.S_new().cpu().numpy())
    for c in (a, b, plain):
        c.close()


def test_run_steps_with_a_hydrostatic_boundary_replays_a_graph_and_equals_step_by_step(hydro):
    """k_hse_fill and its counter inside the captured pair of steps: the stratified atmosphere without gravity (a run with sources
    never reaches the graph), so const_grav = 0 and the column falls; z low is hydrostatic with hse_reflect_vels, which differs
    from the extrapolation of a plain Inflow face as soon as the gas moves.  The batch against step(), bit for bit; the batch's
    one synchronisation has read the counter, which is 0."""
    import castro_amd
    from castro_amd import _lib as L
    from tests.test_ext_bc_cpu import ATMOS
    from tests.test_driver_cpu import _hse_atmosphere
    n, nsteps = (8, 8, 32), 10
    ext = L.make_ext_bc(zl="hse", hse_reflect_vels=1)
    kw = dict(ATMOS, do_grav=False)

    def make(e):
        c = castro_amd.Castro(n, params=L.default_params(), hydro=hydro, ext_bc=e, use_retry=False, **kw)
        c.set_state(_hse_atmosphere(n))
        return c
    a, b, plain = make(ext), make(ext), make(None)
    assert a.host_free_ok() and a.ext_bc.const_grav == 0.0
    for _ in range(nsteps):
        a.step(1.0)
        plain.step(1.0)
    b.run_steps(nsteps, 1.0)
    assert getattr(b, "_graph_error", None) is None and len(b._graphs) > 0, "the batch was not replayed from a graph"
    assert b.nstep == a.nstep == nsteps and b.time == a.time
    assert int(b._unconverged.item()) == 0
    Sa, Sb = a.S_new().cpu().numpy(), b.S_new().cpu().numpy()
    assert np.array_equal(Sa, Sb)
    assert not np.array_equal(Sa, plain.S_new().cpu().numpy())
    for c in (a, b, plain):
        c.close()


def test_run_steps_raises_for_columns_that_did_not_converge_in_the_batch(hydro):
    """the host-free batch reads the counter at its one synchronisation: a count left on the device raises there, naming the face,
    and is cleared"""
    import castro_amd
    from castro_amd import _lib as L
    from tests.test_ext_bc_cpu import ATMOS
    from tests.test_driver_cpu import _hse_atmosphere
    n = (8, 8, 32)
    c = castro_amd.Castro(n, params=L.default_params(), hydro=hydro, ext_bc=L.make_ext_bc(zl="hse"), use_retry=False,
                          **dict(ATMOS, do_grav=False))
    c.set_state(_hse_atmosphere(n))
    assert c.host_free_ok()
    issue = c._step_device

    def step_device(stop_time):
        issue(stop_time)
        c._unconverged.fill_(3)                 # as three walks of this step's fills would leave it, behind them on the stream
    c._step_device = step_device
    with pytest.raises(RuntimeError, match="z-low.*3 ghost columns"):
        c.run_steps(2, 1.0)                     # below the graph's threshold: the steps go out through _step_device
    assert c.nstep == 2 and int(c._unconverged.item()) == 0
    c.close()


def test_amr_patch_on_the_hydrostatic_boundary_equals_its_cpu_twin(hydro, oracle):
    from castro_amd import _lib as L
    from tests.test_ext_bc_cpu import _amr_atmosphere
    ext = L.make_ext_bc(zl="hse")
    cpu = _amr_atmosphere(oracle, ext)
    import castro_amd
    dev = _amr_atmosphere(oracle, ext, backend=lambda: castro_amd.HipHydro(0, numerics=hydro.numerics), params=L.default_params())
    for _ in range(4):
        d_cpu, d_dev = cpu.step(1.0), dev.step(1.0)
        if hydro.numerics == "exact":
            assert d_cpu == d_dev
    for l in (0, 1):
        _close(hydro, dev.levels[l].S_new().cpu().numpy(), cpu.levels[l].S_new().numpy(), "CastroAmr(ext_bc) level %d" % l, bits=False)

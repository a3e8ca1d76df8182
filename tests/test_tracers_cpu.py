"""Tracer particles (castro_amd/particles.py, Castro(tracers=...), CastroAmr(tracers=...)) on the CPU backend with the numpy
restatement of the particle kernels (tests/tracer_backend.py over tests/tracer_ref.py): the input forms, a uniform flow, an
outflow face, the AMR schedule and the level / grid bookkeeping, the timestamp file, particle_count, and passivity."""

import numpy as np
import pytest

from tests import tracer_ref as R
from tests.oracle_backend import OracleBackend
from tests.tracer_backend import TracerOracleBackend

EPS = 2.0 ** -52
PATCH = ((4, 4, 4), (11, 11, 11))           # level-1 zones 8..23: [0.25, 0.75)^3 of the unit domain


def _uniform_state(n, rho, u, e=1.0):
    U = np.zeros((8,) + tuple(n[::-1]))
    U[0] = rho
    for d in range(3):
        U[1 + d] = rho * u[d]
    U[5] = rho * e
    U[4] = rho * e + 0.5 * rho * sum(x * x for x in u)
    U[6] = 1.0
    U[7] = rho
    return U


def _timestamp_lines(tr):
    with open(tr.timestamp_file) as f:
        return [ln.split() for ln in f]


class _Stub:
    """a communicator of two ranks, as far as a constructor looks"""
    rank, size = 0, 2


# ---- 1. the input forms --------------------------------------------------------------------------------------------------------
def test_init_file_ids_ascii_round_trip_and_errors(oracle, tmp_path):
    import castro_amd
    rng = np.random.default_rng(11)
    pos = rng.uniform(0.05, 0.95, size=(7, 3))
    path = tmp_path / "particles.init"
    path.write_text("7\n" + "".join("%.17g %.17g %.17g\n" % tuple(p) for p in pos))
    tr = castro_amd.TracerParticles(init_file=str(path))
    assert tr.n == 7 and np.array_equal(tr.initial_positions, pos)
    c = castro_amd.Castro((16, 16, 16), hydro=TracerOracleBackend(), params=oracle.default_params(), tracers=tr)
    c.initData("sedov", r_init=0.1, nsub=4)
    assert tr.ids().tolist() == list(range(1, 8)) and tr.num_valid == 7
    assert np.array_equal(tr.positions(), pos) and tr.levels().tolist() == [0] * 7
    out = tmp_path / "particles.out"
    tr.write_ascii(str(out))
    rows = out.read_text().split("\n")
    assert int(rows[0]) == 7
    got = np.array([[float(x) for x in r.split()] for r in rows[1:8]])
    assert got.shape == (7, 8) and np.array_equal(got[:, :3], pos)                  # 17 digits round-trip a double
    assert got[:, 6].tolist() == list(range(1, 8)) and not got[:, 7].any() and not got[:, 3:6].any()
    # the round trip: what write_ascii wrote, cut to x y z, is an init file of the same particles
    again = tmp_path / "again.init"
    again.write_text(rows[0] + "\n" + "".join(" ".join(r.split()[:3]) + "\n" for r in rows[1:8]))
    assert np.array_equal(castro_amd.TracerParticles(init_file=str(again)).initial_positions, pos)

    kw = dict(hydro=TracerOracleBackend(), params=oracle.default_params())
    with pytest.raises(ValueError, match="outside the domain"):
        castro_amd.Castro((16, 16, 16), tracers=castro_amd.TracerParticles(positions=[[0.5, 1.0, 0.5]]), **kw)
    # ... a periodic direction wraps instead
    c = castro_amd.Castro((16, 16, 16), lo_bc=(2, 0, 2), hi_bc=(2, 0, 2), tracers=castro_amd.TracerParticles(positions=[[0.5, 1.25, 0.5]]), **kw)
    c.initData("sedov", r_init=0.1, nsub=4)
    assert c.tracers.positions().tolist() == [[0.5, 0.25, 0.5]]
    with pytest.raises(ValueError, match="shape"):
        castro_amd.TracerParticles(positions=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="either"):
        castro_amd.TracerParticles(positions=pos, init_file=str(path))
    with pytest.raises(ValueError, match="either"):
        castro_amd.TracerParticles()
    with pytest.raises(NotImplementedError, match="more than one rank"):
        castro_amd.Castro((16, 16, 16), comm=_Stub(), tracers=castro_amd.TracerParticles(positions=pos), **kw)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        castro_amd.CastroAmr((16, 16, 16), PATCH, comm=_Stub(), make_hydro=TracerOracleBackend, params=oracle.default_params(),
                             tracers=castro_amd.TracerParticles(positions=pos))


# ---- 2. uniform flow -----------------------------------------------------------------------------------------------------------
def test_uniform_flow_positions(oracle):
    """x0 + u t, wrapped, to 8 ulp of the domain length after 5 steps.  Per step and direction the midpoint rule adds two
    roundings of the position (one per pass) and the error of the interpolated velocity times dt; the eight weights sum to 1
    only to rounding: |v - u| <= 12 ulp(u) (seven additions, three products per term), with |u| dt < dx / 2 = 1/32 of the
    length that is well under one ulp of the length per step, as are the wraps.  5 steps x (2 + small) ulp(1) / 2 on average;
    the restatement run below is asserted against the same bound first."""
    import castro_amd
    n, rho, u = (16, 16, 16), 1.3, (0.7, -0.4, 0.25)
    rng = np.random.default_rng(5)
    pos = rng.uniform(0.0, 1.0, size=(64, 3))
    pos[:3] = [[0.999, 0.0005, 0.5], [0.5, 0.5, 0.5], [0.03125, 0.96875, 0.0]]      # next to the wrap, zone centres, a face
    tr = castro_amd.TracerParticles(positions=pos)
    c = castro_amd.Castro(n, lo_bc=(0, 0, 0), hi_bc=(0, 0, 0), hydro=TracerOracleBackend(), params=oracle.default_params(), tracers=tr)
    c.set_state(_uniform_state(n, rho, u))
    dts = [c.step() for _ in range(5)]

    def wrapped_dist(p):
        d = np.abs(p - (pos + np.array(u) * c.time) % 1.0)
        return np.minimum(d, 1.0 - d)

    # the restatement alone, on an exactly uniform half-time array, with the driver's time steps
    geom = c.geom
    fab = _uniform_state(tuple(x + 8 for x in n), rho, u)
    box = [(fab, ((-4, -4, -4), (19, 19, 19)), ((0, 0, 0), (15, 15, 15)))]
    P, flags = R.particles(pos), np.zeros(2, dtype=np.int32)
    for dt in dts:
        R.advect(P, 0, box, geom, dt, flags)
        R.locate(P, 0, 0, 0, [[box[0][2]]], [geom], flags)
    assert not flags.any()
    ref = np.stack([P["x"], P["y"], P["z"]], axis=1)
    assert wrapped_dist(ref).max() <= 8 * EPS
    got = tr.positions()
    print("uniform flow: largest deviation %.3g ulp of the domain length" % (wrapped_dist(got).max() / EPS))
    assert wrapped_dist(got).max() <= 8 * EPS
    assert ((got >= 0.0) & (got < 1.0)).all() and tr.num_valid == 64
    # the corrector's velocity is u to rounding
    assert np.abs(tr.velocities() - np.array(u)).max() <= 12 * EPS


# ---- 3. an outflow face --------------------------------------------------------------------------------------------------------
def test_particle_leaving_through_an_outflow_face(oracle, tmp_path):
    import castro_amd
    n, rho, u = (16, 16, 16), 1.0, (1.0, 0.0, 0.0)
    tr = castro_amd.TracerParticles(positions=[[0.9955, 0.5, 0.5], [0.4, 0.3, 0.6]], timestamp_dir=str(tmp_path / "ts"))
    c = castro_amd.Castro(n, hydro=TracerOracleBackend(), params=oracle.default_params(init_shrink=0.1), tracers=tr)
    c.set_state(_uniform_state(n, rho, u, e=0.01))
    left_at, history = None, []
    for step in range(1, 7):
        c.step()
        x = 0.9955 + u[0] * c.time
        assert abs(x - 1.0) > 1e-6, "the test's particle must not end a step on the face"
        history.append((step, x >= 1.0, tr.ids().tolist(), tr.num_valid))
        if left_at is None and x >= 1.0:
            left_at = step
    assert left_at is not None and 1 < left_at < 6, "the particle leaves in the middle of the run"
    for step, gone, ids, nv in history:
        assert ids == ([-1, 2] if gone else [1, 2]) and nv == (1 if gone else 2), "invalidated in the step it leaves: %r" % (history,)
    lines = _timestamp_lines(tr)
    assert [int(l[0]) for l in lines] == [1, 2] * (left_at - 1) + [2] * (7 - left_at)
    # the invalid particle is never moved again
    frozen = tr.positions()[0].copy()
    c.step()
    assert np.array_equal(tr.positions()[0], frozen) and frozen[0] >= 1.0


# ---- 4. two levels: bookkeeping and schedule -----------------------------------------------------------------------------------
class _Recording(TracerOracleBackend):
    """keeps what every Redistribute saw and left: (lev_min, lev_max, ngrow, levels before, positions / levels / grids after)"""
    def tracer_locate(self, lev_min, lev_max, ngrow, level_boxes, geoms, tracers, flags, stream=None):
        before = tracers.ints[2].numpy().copy()
        super().tracer_locate(lev_min, lev_max, ngrow, level_boxes, geoms, tracers, flags, stream=stream)
        self.calls.append(("located", lev_min, lev_max, ngrow, before, tracers.pos.numpy().T.copy(), tracers.ints[2].numpy().copy(),
                           tracers.ints[3].numpy().copy(), tracers.ints[0].numpy().copy()))


def _expected_levels(lev_min, ngrow, before, pos):
    """level per particle from the positions: the fixed patch covers the level-1 zones 8..23"""
    cell = np.floor(pos * 32.0).astype(int)
    inside = ((cell >= 8) & (cell <= 23)).all(axis=1)
    near = ((cell >= 8 - ngrow) & (cell <= 23 + ngrow)).all(axis=1)
    want = before.copy()
    act = before >= lev_min
    if lev_min == 0:
        want[act] = np.where(inside[act], 1, 0)
    else:
        assert near[act].all(), "a level-1 particle further than ngrow zones from its level"
        want[act] = 1
    return want


def test_amr_levels_grids_and_schedule(oracle):
    import castro_amd
    pos = [[0.245, 0.5, 0.4], [0.22, 0.45, 0.55], [0.745, 0.5, 0.4], [0.70, 0.3, 0.6], [0.5, 0.5, 0.5], [0.5, 0.1, 0.5],
           [0.99, 0.9, 0.9], [0.2499, 0.26, 0.74]]
    calls = []
    tr = castro_amd.TracerParticles(positions=pos)
    a = castro_amd.CastroAmr((16, 16, 16), PATCH, lo_bc=(0, 0, 0), hi_bc=(0, 0, 0), params=oracle.default_params(init_shrink=1.0),
                             make_hydro=lambda: _Recording(calls=calls), tracers=tr)
    a.initData("sod", rho_l=1.0, u_l=1.0, p_l=0.01, rho_r=1.0, u_r=1.0, p_r=0.01, idir=1, frac=0.5)
    assert tr.levels().tolist() == [0, 0, 1, 1, 1, 0, 0, 0]
    for _ in range(3):
        a.step()
    seq = [c for c in calls if c[0] == "located"]
    assert len(seq) == 1 + 2 * 3
    history = []
    for _, lev_min, lev_max, ngrow, before, p, lev, grid, ids in seq:
        assert lev_max == 1 and (ids > 0).all()
        assert lev.tolist() == _expected_levels(lev_min, ngrow, before, p).tolist()
        assert not grid.any()                                   # one box per level
        history.append(lev.tolist())
    h = np.array(history)
    assert (h[0, :2] == 0).all() and (h[-1, :2] == 1).all(), "coarse -> fine"
    assert (h[0, 2:4] == 1).all() and (h[-1, 2:4] == 0).all(), "fine -> coarse"
    assert (h[:, 4] == 1).all() and (h[:, 5] == 0).all()
    assert (np.abs(tr.positions()[:, 0] - (np.array(pos)[:, 0] + a.time) % 1.0) < 1e-12).all()
    # the reference's schedule, per coarse step
    log = [c for c in calls if c[0] in ("advect", "locate")]
    step = [("advect", 0, 0, 1), ("advect", 0, 1, 1), ("advect", 1, 0, 1), ("advect", 1, 1, 1), ("locate", 1, 1, 1),
            ("advect", 1, 0, 2), ("advect", 1, 1, 2), ("locate", 0, 1, 0)]
    assert log == [("locate", 0, 1, 0)] + step * 3


def test_redistribute_follows_every_regrid(oracle):
    import castro_amd
    rng = np.random.default_rng(3)
    calls = []
    tr = castro_amd.TracerParticles(positions=rng.uniform(0.3, 0.7, size=(12, 3)))
    a = castro_amd.CastroAmr((16, 16, 16), params=oracle.default_params(init_shrink=0.1), make_hydro=lambda: TracerOracleBackend(calls=calls),
                             refine=[("density", "gradient", 0.05), ("rho_E", "relative_gradient", 0.5)], regrid_int=2,
                             n_error_buf=1, blocking_factor=4, tracers=tr)
    inner = a._regrid

    def logged(lbase=0, alpha=1.0):
        changed = inner(lbase, alpha)
        calls.append(("regrid", lbase, len(a.lev) - 1))
        return changed
    a._regrid = logged
    a.initData("sedov", r_init=0.08, nsub=4)
    for _ in range(3):
        a.step()
    at = [i for i, c in enumerate(calls) if c[0] == "regrid"]
    assert at, "the run regrids"
    for i in at:
        _, lbase, finest = calls[i]
        assert calls[i + 1] == ("locate", lbase, finest, 0), calls[i:i + 2]
    assert tr.num_valid == 12 and set(tr.levels().tolist()) <= {0, 1}
    boxes = a._tracer_levels()[0]
    for p, l, g in zip(tr.positions(), tr.levels(), tr.grids()):
        cell = np.floor(p * 16.0 * 2 ** l).astype(int)
        lo, hi = boxes[l][g]
        assert all(lo[d] <= cell[d] <= hi[d] for d in range(3))


# ---- 5. the timestamp file -----------------------------------------------------------------------------------------------------
def test_timestamp_samples_a_linear_density(oracle, tmp_path):
    """rho = 1 + 0.3 x + 0.2 y - 0.25 z at rest with one pressure is a steady state of the scheme; cloud-in-cell interpolation
    reproduces a linear field: eight products and seven additions of terms of size <= 2, 16 ulp(2) at the most, as long as the
    stencil stays off the zones the outflow fill makes (particles at least one zone from the faces)."""
    import castro_amd
    n = (16, 16, 16)
    x = (np.arange(16) + 0.5) / 16.0
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    rho = 1.0 + 0.3 * X + 0.2 * Y - 0.25 * Z
    U = np.zeros((8, 16, 16, 16))
    U[0], U[7] = rho, rho
    U[4] = U[5] = 2.5
    U[6] = 1.0
    rng = np.random.default_rng(8)
    pos = rng.uniform(0.1, 0.9, size=(9, 3))
    tr = castro_amd.TracerParticles(positions=pos, timestamp_dir=str(tmp_path / "ts"), timestamp_temperature=True)
    c = castro_amd.Castro(n, hydro=TracerOracleBackend(), params=oracle.default_params(), tracers=tr)
    c.set_state(U)
    times = []
    for _ in range(3):
        c.step()
        times.append(c.time)
    assert np.array_equal(c.S_new()[0].numpy(), rho), "the state is steady"
    lines = _timestamp_lines(tr)
    assert len(lines) == 3 * 9 and all(len(l) == 8 for l in lines)                  # id cpu x y z time rho T
    T = c.S_new()[6].numpy()
    for k, l in enumerate(lines):
        s, i = divmod(k, 9)
        assert int(l[0]) == i + 1 and int(l[1]) == 0 and float(l[5]) == times[s]
        p = np.array([float(v) for v in l[2:5]])
        assert np.abs(p - pos[i]).max() < 1e-12                                     # nothing moves
        assert abs(float(l[6]) - (1.0 + 0.3 * p[0] + 0.2 * p[1] - 0.25 * p[2])) <= 32 * EPS
        assert T.min() <= float(l[7]) <= T.max()
    assert all("%.17g" % float(v) == v for l in lines for v in l[2:]), "reals with 17 significant digits"


def test_timestamp_fine_particles_twice_per_coarse_step(oracle, tmp_path):
    import castro_amd
    pos = [[0.5, 0.5, 0.5], [0.4, 0.6, 0.45], [0.1, 0.1, 0.1], [0.9, 0.5, 0.5], [0.3, 0.3, 0.7]]
    tr = castro_amd.TracerParticles(positions=pos, timestamp_dir=str(tmp_path / "ts"))
    a = castro_amd.CastroAmr((16, 16, 16), PATCH, params=oracle.default_params(init_shrink=0.1), make_hydro=TracerOracleBackend,
                             tracers=tr)
    a.initData("sedov", r_init=0.1, nsub=4)
    assert tr.levels().tolist() == [1, 1, 0, 0, 1]
    t0 = a.time
    dt = a.step()
    lines = _timestamp_lines(tr)
    # after the first fine subcycle: Timestamp(1): the fine particles at t + dt / 2; at the end: Timestamp(0): level 0, then level 1
    assert [int(l[0]) for l in lines] == [1, 2, 5] + [3, 4] + [1, 2, 5]
    assert [float(l[5]) for l in lines] == [t0 + dt / 2] * 3 + [t0 + dt] * 5
    assert all(len(l) == 7 and float(l[6]) > 0.0 for l in lines)
    a.step()
    assert len(_timestamp_lines(tr)) == 16


# ---- 6. particle_count ---------------------------------------------------------------------------------------------------------
def test_particle_count_field(oracle, tmp_path):
    import castro_amd
    from castro_amd import plotfile
    assert "particle_count" not in plotfile.DERIVE_NAMES
    pos = np.array([[0.5, 0.5, 0.5], [0.51, 0.51, 0.51], [0.4, 0.6, 0.45], [0.1, 0.1, 0.1], [0.9, 0.5, 0.5], [0.3, 0.3, 0.7],
                    [0.1, 0.1, 0.1]])
    tr = castro_amd.TracerParticles(positions=pos)
    a = castro_amd.CastroAmr((16, 16, 16), PATCH, params=oracle.default_params(init_shrink=0.1), make_hydro=TracerOracleBackend,
                             tracers=tr)
    a.initData("sedov", r_init=0.1, nsub=4)
    a.step()
    names = a.writePlotFile(str(tmp_path / "plt_amr"), derive=["pressure", "particle_count"])
    assert names[-1] == "particle_count"
    pf = plotfile.read_plotfile_amr(str(tmp_path / "plt_amr"))
    lev = tr.levels()
    for l in (0, 1):
        cnt = pf["levels"][l]["data"][pf["names"].index("particle_count")]
        assert cnt.sum() == (lev == l).sum() and (cnt == np.round(cnt)).all() and cnt.min() == 0.0
    assert pf["levels"][0]["data"][-1][1, 1, 1] == 2.0 and pf["levels"][1]["data"][-1][8, 8, 8] == 2.0      # two in one zone
    assert "particle_count" not in plotfile.write_plotfile_amr(str(tmp_path / "plt_default"), a)
    # single level, and the request without tracers
    tr1 = castro_amd.TracerParticles(positions=pos)
    c = castro_amd.Castro((16, 16, 16), hydro=TracerOracleBackend(), params=oracle.default_params(), tracers=tr1)
    c.initData("sedov", r_init=0.1, nsub=4)
    c.writePlotFile(str(tmp_path / "plt_one"), derive=["particle_count"])
    one = plotfile.read_plotfile(str(tmp_path / "plt_one"))
    assert one["names"][-1] == "particle_count" and one["data"][-1].sum() == 7 and one["data"][-1][8, 8, 8] == 2.0
    assert "particle_count" not in c.writePlotFile(str(tmp_path / "plt_one_default"))
    plain = castro_amd.Castro((16, 16, 16), hydro=OracleBackend(), params=oracle.default_params())
    plain.initData("sedov", r_init=0.1, nsub=4)
    with pytest.raises(ValueError, match="particle_count"):
        plain.writePlotFile(str(tmp_path / "plt_none"), derive=["particle_count"])


# ---- 7. passivity --------------------------------------------------------------------------------------------------------------
def _sedov_positions():
    return np.random.default_rng(21).uniform(0.2, 0.8, size=(40, 3))


def test_tracers_do_not_change_a_single_level_run(oracle, tmp_path):
    import castro_amd
    runs = []
    for with_tracers in (False, True):
        kw = dict(tracers=castro_amd.TracerParticles(positions=_sedov_positions(), timestamp_dir=str(tmp_path / "ts"),
                                                     timestamp_temperature=True)) if with_tracers else {}
        c = castro_amd.Castro((16, 16, 16), hydro=TracerOracleBackend() if with_tracers else OracleBackend(),
                              params=oracle.default_params(), **kw)
        c.initData("sedov", r_init=0.1, nsub=4)
        dts = [c.step() for _ in range(5)]
        runs.append((dts, c.S_new().numpy().copy(), c))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1].view(np.int64), runs[1][1].view(np.int64))
    tr = runs[1][2].tracers
    assert np.abs(tr.positions() - _sedov_positions()).max() > 0.0 and len(_timestamp_lines(tr)) == 5 * 40
    assert not runs[1][2].host_free_ok()


def test_tracers_do_not_change_a_two_level_run(oracle, tmp_path):
    import castro_amd
    runs = []
    for with_tracers in (False, True):
        kw = dict(tracers=castro_amd.TracerParticles(positions=_sedov_positions(), timestamp_dir=str(tmp_path / "ts"),
                                                     timestamp_temperature=True)) if with_tracers else {}
        a = castro_amd.CastroAmr((16, 16, 16), PATCH, params=oracle.default_params(init_shrink=0.1),
                                 make_hydro=TracerOracleBackend if with_tracers else OracleBackend, **kw)
        a.initData("sedov", r_init=0.1, nsub=4)
        dts = [a.step() for _ in range(5)]
        runs.append((dts, [lev.S_new().numpy().copy() for lev in a.levels], a))
    assert runs[0][0] == runs[1][0]
    for x, y in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    tr = runs[1][2].tracers
    assert set(tr.levels().tolist()) == {0, 1} and np.abs(tr.positions() - _sedov_positions()).max() > 0.0

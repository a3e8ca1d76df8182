"""GPU tests of the tracer particles (castro_amd/csrc/tracer_kernels.hip, Castro(tracers=...), CastroAmr(tracers=...)), for both
numerics builds.  Reference: tests/tracer_ref.py.

Kernel level: the file is compiled without contraction in both builds, so every result is compared with the restatement bit
for bit, flags included.  Driver level, against the same run on the CPU backend: `exact` bit for bit (positions, r, levels,
grids, the timestamp file); `contract`: the state differs within the build's 1e-10, and what that does to a trajectory is
measured -- s = the largest position difference between the CPU run and a CPU run whose half-time arrays carry a random relative
1e-10, bound = max(1e-10 x domain length, 100 s) (the factor 100 is the convention of tests/test_monopole_amr_gpu.py); levels and
grids may differ only for particles within that bound of a box face."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tracer_ref as R

pytestmark = pytest.mark.gpu

_CACHE = {}


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


def _geom(periodic=False):
    from castro_amd import _lib
    bc = (0, 0, 0) if periodic else (2, 2, 2)
    return _lib.make_geom((32, 24, 32), (-1.0, 0.5, 2.0), (0.6, 1.46, 4.0), bc, bc)           # dx = 0.05, 0.04, 0.0625


# ---- the level of three boxes ------------------------------------------------------------------------------------------------
NG = 2
VALID = [((2, 3, 4), (9, 14, 19)), ((10, 3, 4), (17, 14, 19)), ((22, 5, 20), (26, 11, 28))]       # 8x12x16, 8x12x16, 5x7x9
NS = (1, 63, 64, 65, 1000)


def _grown(b, g):
    return tuple(x - g for x in b[0]), tuple(x + g for x in b[1])


def _level():
    if "level" not in _CACHE:
        rng = np.random.default_rng(77)
        boxes = []
        for vb in VALID:
            ab = _grown(vb, NG)
            shp = tuple(ab[1][d] - ab[0][d] + 1 for d in (2, 1, 0))
            fab = rng.uniform(-1.0, 1.0, size=(8,) + shp)
            fab[0] = rng.uniform(0.5, 2.0, size=shp)
            boxes.append((fab, ab, vb))
        geom = _geom()
        vmax = max(np.abs(fab[1:4] / fab[0]).max() for fab, _, _ in boxes)
        dt = 0.45 * min(geom.dx[d] for d in range(3)) / vmax
        _CACHE["level"] = (boxes, geom, dt, vmax)
    return _CACHE["level"]


def _phys(geom, idx):
    """position of the (fractional) zone coordinate idx: zone i spans [i, i + 1)"""
    return [geom.problo[d] + idx[d] * geom.dx[d] for d in range(3)]


def _positions(n, rng, geom):
    """n particles (position, level, grid, valid) cycling through the kinds of the issue"""
    out = []
    kinds = 0
    while len(out) < n:
        k, b = kinds % 9, (kinds // 9) % 3
        kinds += 1
        lo, hi = VALID[b]
        ext = [hi[d] - lo[d] + 1 for d in range(3)]
        if k == 0 or k == 8:                                                      # anywhere in the valid box
            idx = [lo[d] + rng.uniform(0.0, ext[d]) for d in range(3)]
        elif k == 1:                                                              # a corner of the box
            c = rng.integers(0, 2, size=3)
            idx = [lo[d] + c[d] * ext[d] for d in range(3)]
        elif k == 2:                                                              # a face centre
            idx = [lo[d] + 0.5 * ext[d] for d in range(3)]
            d = int(rng.integers(0, 3))
            idx[d] = lo[d] + int(rng.integers(0, 2)) * ext[d]
        elif k == 3:                                                              # a zone centre: f == 0
            idx = [lo[d] + int(rng.integers(0, ext[d])) + 0.5 for d in range(3)]
        elif k == 4:                                                              # within half a zone inside a face
            idx = [lo[d] + rng.uniform(0.0, ext[d]) for d in range(3)]
            d = int(rng.integers(0, 3))
            idx[d] = lo[d] + rng.uniform(0.0, 0.5) if rng.integers(0, 2) else hi[d] + 1 - rng.uniform(0.0, 0.5)
        elif k == 5:                                                              # up to one zone outside the box
            idx = [lo[d] + rng.uniform(0.0, ext[d]) for d in range(3)]
            d = int(rng.integers(0, 3))
            idx[d] = lo[d] - rng.uniform(0.0, 1.0) if rng.integers(0, 2) else hi[d] + 1 + rng.uniform(0.0, 1.0)
        else:
            idx = [lo[d] + rng.uniform(0.0, ext[d]) for d in range(3)]
        out.append((_phys(geom, idx), 1 if k == 6 else 0, b, k != 7))             # k == 6: another level; k == 7: invalid
    return out


def _case(n):
    """(particles before, after pass 0, after pass 1) by the restatement, for N = n; no particle clamps"""
    key = ("case", n)
    if key not in _CACHE:
        boxes, geom, dt, vmax = _level()
        assert vmax * dt < 0.5 * min(geom.dx[d] for d in range(3)), "|v| dt < half a zone everywhere"
        rng = np.random.default_rng(1000 + n)
        spec = _positions(n, rng, geom)
        P = R.particles([s[0] for s in spec])
        P["level"][:] = [s[1] for s in spec]
        P["grid"][:] = [s[2] for s in spec]
        P["id"][[i for i, s in enumerate(spec) if not s[3]]] *= -1
        P["r0"][:], P["r1"][:], P["r2"][:] = rng.normal(size=(3, n))               # what an earlier advance left there
        stages, flags = [R.copy_particles(P)], np.zeros(2, dtype=np.int32)
        for ipass in (0, 1):
            R.advect_pass(P, 0, boxes, geom, dt, ipass, flags)
            stages.append(R.copy_particles(P))
        assert not flags.any(), "the restatement clamps for no particle of the case"
        _CACHE[key] = stages
    return _CACHE[key]


def _device_particles(P):
    from castro_amd import _lib
    pos = _t(np.stack([P["x"], P["y"], P["z"]]))
    r = _t(np.stack([P["r0"], P["r1"], P["r2"]]))
    ints = _t(np.stack([P["id"], P["cpu"], P["level"], P["grid"]]).astype(np.int32))
    return pos, r, ints, _lib.make_tracers(pos, r, ints)


def _same(dev, P, what):
    pos, r, ints = dev[0].cpu().numpy(), dev[1].cpu().numpy(), dev[2].cpu().numpy()
    for k, a in (("x", pos[0]), ("y", pos[1]), ("z", pos[2]), ("r0", r[0]), ("r1", r[1]), ("r2", r[2])):
        assert np.array_equal(a.view(np.int64), P[k].view(np.int64)), "%s: %s differs in %d entries, max %g" % (
            what, k, int((a != P[k]).sum()), np.abs(a - P[k]).max())
    for k, a in (("id", ints[0]), ("cpu", ints[1]), ("level", ints[2]), ("grid", ints[3])):
        assert np.array_equal(a, P[k]), "%s: %s differs" % (what, k)


def _dev_boxes(hydro, boxes):
    fabs = [_t(fab) for fab, _, _ in boxes]
    return hydro.make_tracer_boxes([(vb[0], vb[1], (f, ab)) for f, (_, ab, vb) in zip(fabs, boxes)])


@pytest.mark.parametrize("n", NS)
def test_advect_bits(hydro, n):
    boxes, geom, dt, _ = _level()
    before, mid, after = _case(n)
    dev = _device_particles(before)
    tab = _dev_boxes(hydro, boxes)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    hydro.tracer_advect(0, tab, geom, dt, 0, dev[3], flags)
    torch.cuda.synchronize()
    _same(dev, mid, "pass 0, N = %d" % n)
    hydro.tracer_advect(0, tab, geom, dt, 1, dev[3], flags)
    torch.cuda.synchronize()
    _same(dev, after, "pass 1, N = %d" % n)
    assert flags.tolist() == [0, 0]
    moved = (before["id"] > 0) & (before["level"] == 0)
    assert np.array_equal(after["x"][~moved], before["x"][~moved]) and (n < 9 or (after["x"][moved] != before["x"][moved]).all())


def test_advect_clamps_and_counts(hydro):
    """one more particle, 2.2 zones below box 2 in x: its stencil leaves the array of two ghost zones"""
    boxes, geom, dt, _ = _level()
    before = R.copy_particles(_case(65)[0])
    far = _phys(geom, [VALID[2][0][0] - 2.2, VALID[2][0][1] + 3.3, VALID[2][0][2] + 4.4])
    for k, v in zip("xyz", far):
        before[k][7] = v
    before["id"][7], before["level"][7], before["grid"][7] = 8, 0, 2
    dev = _device_particles(before)
    tab = _dev_boxes(hydro, boxes)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    P, rflags = R.copy_particles(before), np.zeros(2, dtype=np.int32)
    for ipass in (0, 1):
        R.advect_pass(P, 0, boxes, geom, dt, ipass, rflags)
        hydro.tracer_advect(0, tab, geom, dt, ipass, dev[3], flags)
        torch.cuda.synchronize()
        _same(dev, P, "clamped case, pass %d" % ipass)
        assert flags.tolist() == rflags.tolist()
        if ipass == 0:
            assert rflags.tolist() == [1, 0]
    # everything but particle 7 as in the case without it
    clean = _case(65)[2]
    others = np.arange(65) != 7
    assert np.array_equal(P["x"][others], clean["x"][others]) and np.array_equal(P["r2"][others], clean["r2"][others])
    # a grid that is no box of the table: skipped and counted
    before["grid"][7] = 3
    dev = _device_particles(before)
    flags.zero_()
    hydro.tracer_advect(0, tab, geom, dt, 0, dev[3], flags)
    torch.cuda.synchronize()
    assert flags.tolist() == [1, 0] and dev[0][:, 7].cpu().tolist() == far


@pytest.mark.parametrize("comps", [(0,), (6, 0)])
def test_sample_bits(hydro, comps):
    boxes, geom, _, _ = _level()
    for n in (1, 65, 1000):
        P = _case(n)[0]
        dev = _device_particles(P)
        out = torch.full((len(comps), n), -7.0, dtype=torch.float64, device="cuda")
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        hydro.tracer_sample(0, _dev_boxes(hydro, boxes), geom, comps, dev[3], out, flags)
        torch.cuda.synchronize()
        want, rflags = np.full((len(comps), n), -7.0), np.zeros(2, dtype=np.int32)
        R.sample(P, 0, boxes, geom, comps, want, rflags)
        assert np.array_equal(out.cpu().numpy().view(np.int64), want.view(np.int64)) and flags.tolist() == rflags.tolist() == [0, 0]
        _same(dev, P, "sample leaves the particles alone")
        mine = (P["id"] > 0) & (P["level"] == 0)
        assert (want[:, ~mine] == -7.0).all() and (want[:, mine] != -7.0).all()


# ---- Redistribute --------------------------------------------------------------------------------------------------------------
def _locate_case(periodic):
    from castro_amd import _lib
    bc = (0, 0, 0) if periodic else (2, 2, 2)
    g0 = _lib.make_geom((16, 16, 16), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), bc, bc)
    g1 = _lib.make_geom((32, 32, 32), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), bc, bc)
    # level 0: two boxes that tile the domain; level 1: a box nested in them and a second one that overlaps it
    boxes = [[((0, 0, 0), (7, 15, 15)), ((8, 0, 0), (15, 15, 15))], [((8, 8, 8), (23, 23, 23)), ((20, 8, 8), (27, 23, 23))]]
    return [g0, g1], boxes


def _run_locate(hydro, P, geoms, boxes, lev_min, lev_max, ngrow):
    dev = _device_particles(P)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    hydro.tracer_locate(lev_min, lev_max, ngrow, boxes, geoms, dev[3], flags)
    torch.cuda.synchronize()
    Q, rflags = R.copy_particles(P), np.zeros(2, dtype=np.int32)
    R.locate(Q, lev_min, lev_max, ngrow, boxes, geoms, rflags)
    _same(dev, Q, "locate(%d, %d, %d)" % (lev_min, lev_max, ngrow))
    assert flags.tolist() == rflags.tolist()
    return Q, rflags.tolist()


def test_locate_periodic_wrap_levels_and_invalidation(hydro):
    geoms, boxes = _locate_case(True)
    tiny = -2.0 ** -60                      # tiny + 1.0 == 1.0: the wrap lands on probhi and becomes problo
    pos = [[1.3, 0.1, 0.1], [0.1, -0.2, 0.1], [0.1, 0.1, 2.6], [-1.7, 1.0, -0.1],          # wraps, each direction and both ways
           [tiny, 0.3, 0.3], [0.3, tiny, 0.3], [0.3, 0.3, tiny], [1.0, 1.0, 1.0],          # lands on / sits at probhi
           [0.5, 0.5, 0.5], [0.3, 0.5, 0.5], [0.7, 0.5, 0.5], [0.8, 0.5, 0.5], [0.9, 0.5, 0.5]]
    P = R.particles(pos)
    P["id"][8] = -9                          # an invalid one: untouched
    Q, flags = _run_locate(hydro, P, geoms, boxes, 0, 1, 0)
    assert flags == [0, 0]
    assert [Q["x"][4], Q["y"][5], Q["z"][6]] == [0.0, 0.0, 0.0] and [Q[k][7] for k in "xyz"] == [0.0, 0.0, 0.0]
    assert abs(Q["x"][0] - 0.3) < 1e-15 and abs(Q["y"][1] - 0.8) < 1e-15 and abs(Q["z"][2] - 0.6) < 1e-15
    assert abs(Q["x"][3] - 0.3) < 1e-15 and Q["y"][3] == 0.0 and abs(Q["z"][3] - 0.9) < 1e-15
    # finest level wins; the lowest box index of two that hold the zone (x = 0.7: level-1 zone 22 is in both boxes)
    assert list(zip(Q["level"][9:], Q["grid"][9:])) == [(1, 0), (1, 0), (1, 1), (0, 1)]
    assert (Q["level"][8], Q["grid"][8], Q["x"][8]) == (0, 0, 0.5)
    # restricted to level 0
    Q0, _ = _run_locate(hydro, P, geoms, boxes, 0, 0, 0)
    assert list(zip(Q0["level"][9:], Q0["grid"][9:])) == [(0, 0), (0, 1), (0, 1), (0, 1)]
    # non-periodic: outside in one direction invalidates, and only that
    geoms, boxes = _locate_case(False)
    P = R.particles([[1.0, 0.5, 0.5], [0.5, -1e-9, 0.5], [0.5, 0.5, 0.999], [0.0, 0.0, 0.0]])
    Q, flags = _run_locate(hydro, P, geoms, boxes, 0, 1, 0)
    assert Q["id"].tolist() == [-1, -2, 3, 4] and flags == [0, 0] and Q["x"][0] == 1.0


def test_locate_ngrow_fallback_and_lost_flag(hydro):
    geoms, boxes = _locate_case(False)
    one = [boxes[0], boxes[1][:1]]          # level 1: the zones 8..23
    pos = [[0.5, 0.5, 0.5], [0.76, 0.5, 0.5], [0.8, 0.5, 0.5], [0.24, 0.24, 0.5], [0.1, 0.5, 0.5]]
    P = R.particles(pos, level=1)
    P["level"][4] = 0                        # below lev_min: not looked at
    Q, flags = _run_locate(hydro, P, geoms, one, 1, 1, 1)
    assert Q["level"].tolist() == [1, 1, 1, 1, 0] and flags == [0, 1], "0.8 is two zones outside: lost, level and grid stay"
    Q, flags = _run_locate(hydro, P, geoms, one, 1, 1, 2)
    assert flags == [0, 0]
    Q, flags = _run_locate(hydro, P, geoms, one, 1, 1, 0)
    assert flags == [0, 3]
    Q, flags = _run_locate(hydro, P, geoms, one, 0, 1, 0)
    assert Q["level"].tolist() == [1, 0, 0, 0, 0] and Q["grid"].tolist() == [0, 1, 1, 0, 0] and flags == [0, 0]


# ---- particle_count --------------------------------------------------------------------------------------------------------------
def test_count_bits_and_empty_container(hydro):
    boxes, geom, _, _ = _level()
    P = R.copy_particles(_case(1000)[0])
    zone = _phys(geom, [4.5, 6.5, 8.5])
    for t in (0, 9, 18, 27):                # several particles in one zone of box 0
        for k, v in zip("xyz", zone):
            P[k][t] = v + 1e-3 * t * geom.dx[0]
        P["id"][t], P["level"][t], P["grid"][t] = t + 1, 0, 0
    dev = _device_particles(P)
    cnt = [torch.zeros(tuple(vb[1][d] - vb[0][d] + 1 for d in (2, 1, 0)), dtype=torch.int32, device="cuda") for _, _, vb in boxes]
    tab = hydro.make_tracer_boxes([(vb[0], vb[1], (c, vb)) for c, (_, _, vb) in zip(cnt, boxes)])
    hydro.tracer_count(0, tab, geom, dev[3])
    torch.cuda.synchronize()
    want = [(np.zeros(tuple(c.shape), dtype=np.int32), vb) for c, (_, _, vb) in zip(cnt, boxes)]
    R.count(P, 0, want, geom)
    for c, (w, _) in zip(cnt, want):
        assert np.array_equal(c.cpu().numpy(), w)
    assert want[0][0][8 - 4, 6 - 3, 4 - 2] >= 4 and sum(int(w.sum()) for w, _ in want) > 400
    _same(dev, P, "count leaves the particles alone")
    # N = 0: nothing is launched, every call returns OK
    E = R.particles(np.zeros((0, 3)))
    edev = _device_particles(E)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    for c in cnt:
        c.zero_()
    hydro.tracer_count(0, tab, geom, edev[3])
    hydro.tracer_advect(0, _dev_boxes(hydro, boxes), geom, 0.1, 0, edev[3], flags)
    hydro.tracer_sample(0, _dev_boxes(hydro, boxes), geom, (0,), edev[3], torch.zeros((1, 0), dtype=torch.float64, device="cuda"), flags)
    hydro.tracer_locate(0, 0, 0, [[vb for _, _, vb in boxes]], [geom], edev[3], flags)
    torch.cuda.synchronize()
    assert flags.tolist() == [0, 0] and not any(int(c.sum()) for c in cnt)


# ---- argument errors -----------------------------------------------------------------------------------------------------------
def test_argument_checks(hydro):
    from castro_amd import _lib
    boxes, geom, dt, _ = _level()
    P = _case(64)[0]
    dev = _device_particles(P)
    tab = _dev_boxes(hydro, boxes)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    bad = _lib.Geom.from_buffer_copy(geom)
    bad.coord = 1
    with pytest.raises(RuntimeError, match="unsupported"):
        hydro.tracer_advect(0, tab, bad, dt, 0, dev[3], flags)
    with pytest.raises(RuntimeError, match="unsupported"):
        hydro.tracer_sample(0, tab, bad, (0,), dev[3], torch.zeros((1, 64), dtype=torch.float64, device="cuda"), flags)
    with pytest.raises(RuntimeError, match="unsupported"):
        hydro.tracer_locate(0, 0, 0, [[vb for _, _, vb in boxes]], [bad], dev[3], flags)
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.tracer_advect(0, tab, geom, dt, 2, dev[3], flags)                   # no such pass
    three = [_t(fab[:3]) for fab, _, _ in boxes]                                  # ncomp < 4: no z momentum
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.tracer_advect(0, hydro.make_tracer_boxes([(vb[0], vb[1], (f, ab)) for f, (_, ab, vb) in zip(three, boxes)]), geom, dt, 0,
                            dev[3], flags)
    with pytest.raises(RuntimeError, match="bad argument"):                       # component 6 of a 3-component FAB
        hydro.tracer_sample(0, hydro.make_tracer_boxes([(vb[0], vb[1], (f, ab)) for f, (_, ab, vb) in zip(three, boxes)]), geom, (6,),
                            dev[3], torch.zeros((1, 64), dtype=torch.float64, device="cuda"), flags)
    nul = _lib.Tracers.from_buffer_copy(dev[3])
    nul.grid = None
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.tracer_advect(0, tab, geom, dt, 0, nul, flags)
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.tracer_locate(0, 1, 0, [[vb for _, _, vb in boxes]], [geom], dev[3], flags)          # lev_max beyond the levels
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.tracer_locate(0, 0, -1, [[vb for _, _, vb in boxes]], [geom], dev[3], flags)
    wrong = hydro.make_tracer_boxes([(vb[0], vb[1], (_t(fab[:2]), ab)) for fab, ab, vb in boxes])   # a count FAB has one component
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.tracer_count(0, wrong, geom, dev[3])
    rc = hydro.lib.castro_amd_tracer_advect_mf(hydro.h, 0, tab[1], tab[0], C.byref(geom), dt, 0, C.byref(dev[3]), None, None)
    assert rc == _lib.ERR_ARG                                                     # no flags
    torch.cuda.synchronize()
    _same(dev, P, "a refused call writes nothing")
    assert flags.tolist() == [0, 0]


# ---- the drivers ---------------------------------------------------------------------------------------------------------------
PATCH = ((4, 4, 4), (11, 11, 11))


def _tracer_positions():
    rng = np.random.default_rng(31)
    pos = rng.uniform(0.3, 0.7, size=(200, 3))
    pos[:20] = rng.uniform(0.05, 0.95, size=(20, 3))
    return pos


def _snapshot(tr):
    with open(tr.timestamp_file) as f:
        text = f.read()
    return dict(pos=tr.positions(), r=tr.velocities(), level=tr.levels(), grid=tr.grids(), id=tr.ids(), text=text)


def _single(make_hydro, params, tmp, **kw):
    import castro_amd
    tr = castro_amd.TracerParticles(positions=_tracer_positions(), timestamp_dir=str(tmp), timestamp_temperature=True)
    c = castro_amd.Castro((16, 16, 16), hydro=make_hydro(), params=params, tracers=tr, **kw)
    c.initData("sedov", r_init=0.1, nsub=4)
    for _ in range(5):
        c.step()
    return _snapshot(tr), [[(c.lo, c.hi)]], [c.geom]


def _two_level(make_hydro, params, tmp):
    import castro_amd
    tr = castro_amd.TracerParticles(positions=_tracer_positions(), timestamp_dir=str(tmp), timestamp_temperature=True)
    a = castro_amd.CastroAmr((16, 16, 16), PATCH, params=params, make_hydro=make_hydro, tracers=tr)
    a.initData("sedov", r_init=0.1, nsub=4)
    for _ in range(2):
        a.step()
    return _snapshot(tr), a._tracer_levels()[0], a._tracer_levels()[1]


def _cpu_runs(kind, oracle, tmp_path_factory):
    """the run on the CPU backend and its perturbed twin, once for both builds"""
    if kind not in _CACHE:
        from tests.tracer_backend import TracerOracleBackend
        run = _single if kind == "single" else _two_level
        P = oracle.default_params(init_shrink=0.1)
        ref = run(TracerOracleBackend, P, tmp_path_factory.mktemp(kind + "_cpu"))
        seeds = iter(range(100))
        twin = run(lambda: TracerOracleBackend(perturb=1e-10, seed=next(seeds)), P, tmp_path_factory.mktemp(kind + "_twin"))
        _CACHE[kind] = (ref, float(np.abs(twin[0]["pos"] - ref[0]["pos"]).max()))
    return _CACHE[kind]


def _face_distance(pos, level_boxes, geoms):
    """per particle, the distance to the nearest box face of any level (in the units of the positions)"""
    d = np.full(pos.shape[0], np.inf)
    for bl, g in zip(level_boxes, geoms):
        for lo, hi in bl:
            for k in range(3):
                for face in (g.problo[k] + lo[k] * g.dx[k], g.problo[k] + (hi[k] + 1) * g.dx[k]):
                    d = np.minimum(d, np.abs(pos[:, k] - face))
    return d


def _compare(hydro, got, cpu, what):
    (ref, level_boxes, geoms), s = cpu
    assert np.array_equal(got["id"], ref["id"])
    if hydro.numerics == "exact":
        for k in ("pos", "r"):
            assert np.array_equal(got[k].view(np.int64), ref[k].view(np.int64)), "%s: %s differs, max %g" % (
                what, k, np.abs(got[k] - ref[k]).max())
        assert np.array_equal(got["level"], ref["level"]) and np.array_equal(got["grid"], ref["grid"])
        assert got["text"] == ref["text"], "%s: the timestamp files differ" % what
        return
    bound = max(1e-10 * 1.0, 100.0 * s)
    dev = np.abs(got["pos"] - ref["pos"]).max()
    print("%s (contract): largest position deviation / bound = %.3g (s = %.3g)" % (what, dev / bound, s))
    assert dev <= bound
    moved = (got["level"] != ref["level"]) | (got["grid"] != ref["grid"])
    assert (_face_distance(ref["pos"], level_boxes, geoms)[moved] <= bound).all(), \
        "levels and grids differ only for particles within the bound of a box face"
    assert len(got["text"].splitlines()) == len(ref["text"].splitlines())


def test_single_level_driver_against_the_cpu_run(hydro, oracle, tmp_path_factory):
    from castro_amd import _lib
    cpu = _cpu_runs("single", oracle, tmp_path_factory)
    got = _single(lambda: hydro, _lib.default_params(init_shrink=0.1), tmp_path_factory.mktemp("single_gpu"))[0]
    torch.cuda.synchronize()
    assert (np.abs(got["pos"] - _tracer_positions()).max(axis=1) > 0.0).any()
    _compare(hydro, got, cpu, "Castro 16^3 Sedov, 5 steps")


def test_two_level_driver_against_the_cpu_run(hydro, oracle, tmp_path_factory):
    import castro_amd
    from castro_amd import _lib
    cpu = _cpu_runs("amr", oracle, tmp_path_factory)
    got = _two_level(lambda: castro_amd.HipHydro(0, numerics=hydro.numerics), _lib.default_params(init_shrink=0.1),
                     tmp_path_factory.mktemp("amr_gpu"))[0]
    torch.cuda.synchronize()
    assert set(got["level"].tolist()) == {0, 1}
    _compare(hydro, got, cpu, "CastroAmr 16^3 + patch Sedov, 2 coarse steps")

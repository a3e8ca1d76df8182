"""GPU tests of checkpoint / restart: the pack launch (k_fab_pack_minmax / k_fab_minmax_final of castro_amd/csrc/checkpoint_kernels.hip
behind castro_amd_fab_pack / castro_amd_fab_unpack) against torch slicing, and the drivers' continuation on the device, for both
numerics builds.  Every comparison is bitwise: a copy and a comparison have no rounding, and a restarted run issues the kernels
of the uninterrupted one on the same values."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest
import torch

from tests.test_checkpoint_cpu import compare_amr, compare_single, continuation

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


def _eq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _fab(rng, lo, n, ncomp, g, fill):
    """(tensor, box, (lo, hi)): a FAB of `ncomp` components on the box [lo, lo + n) grown by g, its ghost zones holding `fill`,
    its valid zones random values in (1, 2)"""
    hi = tuple(lo[d] + n[d] - 1 for d in range(3))
    box = (tuple(x - g for x in lo), tuple(x + g for x in hi))
    t = np.full((ncomp, n[2] + 2 * g, n[1] + 2 * g, n[0] + 2 * g), fill)
    t[:, g:g + n[2], g:g + n[1], g:g + n[0]] = rng.uniform(1.0, 2.0, size=(ncomp, n[2], n[1], n[0]))
    return t, box, (lo, hi)


def _valid(t, box, reg):
    lo, hi = reg
    o = box[0]
    return t[:, lo[2] - o[2]:hi[2] - o[2] + 1, lo[1] - o[1]:hi[1] - o[1] + 1, lo[0] - o[0]:hi[0] - o[0] + 1]


# ---- 9. pack against torch slicing --------------------------------------------------------------------------------------------
def _five_entries():
    rng = np.random.default_rng(901)
    shapes = [((8, 8, 8), 8, 4, 1e300), ((5, 3, 7), 7, 3, -1e300), ((16, 8, 12), 3, 1, np.nan), ((1, 1, 9), 1, 0, 0.0),
              ((33, 2, 2), 8, 4, np.nan)]
    los = [(3, -2, 5), (-7, 11, 2), (100, 40, -9), (1, 2, 3), (-33, -2, 64)]            # no box at the origin
    fabs = [_fab(rng, lo, n, nc, g, fill) for lo, (n, nc, g, fill) in zip(los, shapes)]
    v0 = _valid(*fabs[0])
    v0[0, 0, 0, 0] = 0.25                       # the minimum of a component in the first valid zone,
    v0[1, -1, -1, -1] = 0.125                   # of another in the last,
    v0[2, 0, -1, -1] = -3.0                     # of a third next to a ghost corner (x and y at their upper ends, z at its lower)
    v0[3, -1, 0, 0] = 7.0                       # and a maximum next to another
    v2 = _valid(*fabs[2])
    v2[0, 3, 2, 5] = 5e-324                     # a denormal as the minimum of a component
    v2[1, 0, 0, 0] = -5e-324                    # and -denormal
    v3 = _valid(*fabs[3])
    v3[0, 4, 0, 0] = -0.0                       # -0.0 as the minimum of positive values
    return fabs


def test_pack_against_torch_slicing(hydro):
    fabs = _five_entries()
    dev = [(torch.from_numpy(t).cuda(), box, reg) for t, box, reg in fabs]
    entries = hydro.make_pack_entries(dev)
    _, n, doubles, pairs = entries
    assert (n, pairs) == (5, 8 + 7 + 3 + 1 + 8) and doubles == sum(_valid(*f).size for f in fabs)
    want = torch.cat([_valid(*f).reshape(-1) for f in dev])
    flat = [_valid(*f).reshape(f[0].shape[0], -1) for f in dev]
    want_mm = torch.cat([x.amin(dim=1) for x in flat] + [x.amax(dim=1) for x in flat])
    dst = torch.full((doubles + 3,), 777.0, dtype=torch.float64, device="cuda")
    mm = torch.full((2 * pairs + 2,), 777.0, dtype=torch.float64, device="cuda")
    hydro.fab_pack(entries, dst, mm)
    torch.cuda.synchronize()
    assert _eq(dst[:doubles], want) and bool((dst[doubles:] == 777.0).all())
    assert _eq(mm[:2 * pairs], want_mm) and bool((mm[2 * pairs:] == 777.0).all())
    assert mm[0].item() == 0.25 and mm[1].item() == 0.125 and mm[2].item() == -3.0 and mm[pairs + 3].item() == 7.0
    assert mm[15].item() == 5e-324 and mm[16].item() == -5e-324
    m3 = mm[18].item()
    assert m3 == 0.0 and np.signbit(m3)         # -0.0
    # without the min / max vector: the copy alone
    dst2 = torch.full_like(dst, 777.0)
    hydro.fab_pack(entries, dst2)
    torch.cuda.synchronize()
    assert _eq(dst2, dst)
    # the two builds give the same bits
    got = (dst.cpu(), mm.cpu())
    other = _CACHE.setdefault("pack", (hydro.numerics, got))
    if other[0] != hydro.numerics:
        assert _eq(other[1][0], got[0]) and _eq(other[1][1], got[1])


def test_nan_in_a_valid_zone_propagates_into_min_and_max(hydro):
    """the rule of tests/test_checkpoint_cpu.py on the device: NaN in the first zone of a component, in the middle of another (so
    that it meets the running value from both sides and crosses lanes, waves and workgroups), and a component that is all NaN;
    every other pair keeps its bits"""
    rng = np.random.default_rng(902)
    fabs = [_fab(rng, (3, -2, 5), (40, 40, 12), 3, 2, 1e300), _fab(rng, (-7, 11, 2), (5, 3, 7), 2, 1, -1e300),
            _fab(rng, (0, 0, 64), (6, 6, 6), 2, 0, 0.0)]
    _valid(*fabs[0])[1, 5, 17, 23] = np.nan
    _valid(*fabs[1])[0, 0, 0, 0] = np.nan
    _valid(*fabs[2])[1] = np.nan
    dev = [(torch.from_numpy(t).cuda(), box, reg) for t, box, reg in fabs]
    entries = hydro.make_pack_entries(dev)
    _, n, doubles, pairs = entries
    dst = torch.empty(doubles, dtype=torch.float64, device="cuda")
    mm = torch.empty(2 * pairs, dtype=torch.float64, device="cuda")
    hydro.fab_pack(entries, dst, mm)
    torch.cuda.synchronize()
    flat = [_valid(*f).reshape(f[0].shape[0], -1) for f in dev]
    want = torch.cat([x.amin(dim=1) for x in flat] + [x.amax(dim=1) for x in flat])
    nan = torch.isnan(want)
    assert nan.cpu().tolist() == [False, True, False, True, False, False, True] * 2
    assert torch.equal(torch.isnan(mm), nan) and _eq(mm[~nan], want[~nan])
    assert _eq(dst, torch.cat([x.reshape(-1) for x in flat]))             # the copy carries the NaNs with their bits


# ---- 10. round trip and many boxes -------------------------------------------------------------------------------------------
def _round_trip(hydro, fabs):
    SENT = -12345.0
    dev = [(torch.from_numpy(t).cuda(), box, reg) for t, box, reg in fabs]
    entries = hydro.make_pack_entries(dev)
    _, n, doubles, pairs = entries
    buf = torch.empty(doubles, dtype=torch.float64, device="cuda")
    mm = torch.empty(2 * pairs, dtype=torch.float64, device="cuda")
    hydro.fab_pack(entries, buf, mm)
    back = [(torch.full_like(t, SENT), box, reg) for t, box, reg in dev]
    hydro.fab_unpack(hydro.make_pack_entries(back), buf)
    torch.cuda.synchronize()
    flat = [_valid(*f).reshape(f[0].shape[0], -1) for f in dev]
    assert _eq(buf, torch.cat([x.reshape(-1) for x in flat]))
    assert _eq(mm, torch.cat([x.amin(dim=1) for x in flat] + [x.amax(dim=1) for x in flat]))
    for (t, box, reg), (u, _, _) in zip(dev, back):
        assert _eq(_valid(u, box, reg), _valid(t, box, reg))
        ghost = torch.ones_like(u, dtype=torch.bool)
        _valid(ghost, box, reg)[...] = False
        assert bool((u[ghost] == SENT).all())                               # every ghost zone is left at the sentinel


def test_round_trip_many_boxes(hydro):
    """70 entries of 4 x 4 x 4 in one call: more than one wave of entries, more than 64 prefix elements; ghost widths 1 and 2
    alternate, so both the one-zone and the two-zone form of the copy run"""
    rng = np.random.default_rng(1001)
    fabs = [_fab(rng, (4 * (i % 7) - 9, 4 * (i // 7) + 1, 3 * i - 50), (4, 4, 4), 3 + i % 2, 1 + i % 2, float(i)) for i in range(70)]
    _round_trip(hydro, fabs)


def test_round_trip_one_large_box(hydro):
    """one entry of 64 x 64 x 64 in one call: many workgroups per component"""
    rng = np.random.default_rng(1002)
    _round_trip(hydro, [_fab(rng, (-8, 16, 64), (64, 64, 64), 2, 4, np.nan)])


# ---- 11. arguments --------------------------------------------------------------------------------------------------------------
def test_arguments(hydro):
    from castro_amd import _lib as L
    lib, h = hydro.lib, hydro.h
    rng = np.random.default_rng(1101)
    t, box, reg = _fab(rng, (2, 2, 2), (4, 4, 4), 2, 1, 9.0)
    d = torch.from_numpy(t).cuda()
    buf = torch.zeros(2 * 64, dtype=torch.float64, device="cuda")
    mm = torch.zeros(4, dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    good = lambda: hydro.make_pack_entries([(d, box, reg)])[0]
    hydro.profile(True)
    hydro.profile_reset()
    pack = lambda n, e, dst, m=None: lib.castro_amd_fab_pack(h, n, e, dst, m, None)
    unpack = lambda n, e, src: lib.castro_amd_fab_unpack(h, n, e, src, None)
    assert pack(0, None, None) == L.OK and unpack(0, None, None) == L.OK              # n == 0: a no-op
    assert pack(0, good(), p(buf), p(mm)) == L.OK
    for call in (pack, unpack):
        assert call(-1, good(), p(buf)) == L.ERR_ARG
        assert call(1, None, p(buf)) == L.ERR_ARG and call(1, good(), None) == L.ERR_ARG
        e = good()
        e[0].vhi[0] = box[1][0] + 1                                                 # a valid region outside its box
        assert call(1, e, p(buf)) == L.ERR_ARG
        e = good()
        e[0].vlo[2] = box[0][2] - 1
        assert call(1, e, p(buf)) == L.ERR_ARG
        e = good()
        e[0].fab.ncomp = 0
        assert call(1, e, p(buf)) == L.ERR_ARG
        e = good()
        e[0].fab.p = None
        assert call(1, e, p(buf)) == L.ERR_ARG
    torch.cuda.synchronize()
    assert not [k for k in hydro.profile_report() if k.startswith("k_fab")], "nothing is launched for a refused call"
    assert bool((buf == 0.0).all()) and bool((d == torch.from_numpy(t).cuda()).all())
    assert pack(1, good(), p(buf), p(mm)) == L.OK                                   # the good table is good
    torch.cuda.synchronize()
    rep = hydro.profile_report()
    assert rep["k_fab_pack_minmax"][1] == 1 and rep["k_fab_minmax_final"][1] == 1
    hydro.profile(False)
    with pytest.raises(ValueError):
        hydro.fab_pack(hydro.make_pack_entries([(d, box, reg)]), buf[:100])       # the wrapper checks the size of the buffer


# ---- 12. continuation on the device --------------------------------------------------------------------------------------------
def _sedov32(hydro, **kw):
    import castro_amd
    return lambda: castro_amd.Castro((32, 32, 32), hydro=hydro, params=castro_amd.default_params(), **kw)


def _init(c):
    c.initData("sedov", r_init=0.1, nsub=4)


def test_continuation_sedov_step(hydro, tmp_path):
    a, c, d = continuation(_sedov32(hydro), _init, tmp_path)
    assert hasattr(hydro, "fab_pack")


def test_continuation_sedov_step_graph(hydro, tmp_path):
    """through run_steps with the step graph: the checkpoint lies between two batches, the restarted object captures its own"""
    make = _sedov32(hydro)
    a, c, d = continuation(make, _init, tmp_path, nsteps=2, at=1, step=lambda x: x.run_steps(4))
    assert a.nstep == 8 and c.host_free_ok() and len(c._graphs) >= 1 and len(a._graphs) >= 1
    # and through evolve: batches that end on the multiples of check_int
    b = make()
    _init(b)
    b.check_int, b.check_file = 4, str(tmp_path / "ev")
    b.evolve(a.time + 1.0, max_step=8)
    b.close()
    assert sorted(x for x in os.listdir(str(tmp_path)) if x.startswith("ev")) == ["ev00004", "ev00008"]
    compare_single(a, b, bookkeeping=False)
    e = make()
    e.restart(str(tmp_path / "ev00004"))
    e.evolve(a.time + 1.0, max_step=8)
    compare_single(b, e)


def test_continuation_gravity_predictor(hydro, tmp_path):
    import castro_amd
    make = lambda: castro_amd.Castro((16, 16, 16), hydro=hydro, params=castro_amd.default_params(source_term_predictor=1), do_grav=True,
                                     const_grav=-1.0)
    a, _, _ = continuation(make, _init, tmp_path)
    assert float(a.new_source.abs().max()) > 0.0


def test_continuation_dust_collapse_point_mass_tracers(hydro, tmp_path):
    import castro_amd
    from tests import monopole_ref as R
    pos = np.random.default_rng(1201).uniform(0.1, 0.9, size=(50, 3)) * 7.5e8

    def make():
        c = castro_amd.Castro(R.DUST_N, hydro=hydro, params=castro_amd.default_params(**R.DUST_PARAMS), do_grav=True,
                              gravity_type="monopole", drdxfac=R.DUST_DRDXFAC, use_point_mass=True, point_mass=1.e30,
                              point_mass_fix_solution=True, tracers=castro_amd.TracerParticles(positions=pos), **R.DUST_GEOM)
        c.center = (0.0, 0.0, 0.0)
        return c
    a, c, d = continuation(make, lambda x: x.initData("dust_collapse", **R.DUST_PROB), tmp_path)
    assert a.point_mass != 1.e30 and sorted(os.listdir(os.path.join(d, "Particles"))) == ["DATA_00000", "Header"]
    assert open(os.path.join(d, "point_mass")).read() != "%.17g\n" % 1.e30


def test_continuation_amr_batched(hydro, tmp_path):
    import castro_amd
    make = lambda: castro_amd.CastroAmr((16, 16, 16), max_level=1, refine=[("density", "gradient", 0.01)], regrid_int=2,
                                        params=castro_amd.default_params(init_shrink=1.0),
                                        make_hydro=lambda: castro_amd.HipHydro(0, numerics=hydro.numerics))
    init = lambda x: x.initData("sod", rho_l=1.0, u_l=0.0, p_l=1.0, rho_r=0.125, u_r=0.0, p_r=0.1)
    a, c, d = continuation(make, init, tmp_path, nsteps=4, at=2, compare=compare_amr)
    assert len(a.lev) == 2 and a.lev[1].batched and c.lev[1].batched and c.level_count[:2] == [2, 4]


# ---- 13. background write during steps -----------------------------------------------------------------------------------------
def test_background_write_during_steps(hydro, tmp_path):
    """writeCheckpoint(background=True) after step 2, two more steps at once, checkpoint_wait(): the directory equals, file by
    file, the one a synchronous writeCheckpoint of an identical run wrote at step 2 -- CPUtime apart, which holds the wall time of
    the run and is compared as a number of 17 significant digits --, and the state at step 4 equals the run without a checkpoint"""
    make = _sedov32(hydro)
    runs = []
    for k in range(3):
        c = make()
        _init(c)
        c.step(), c.step()
        runs.append(c)
    x, y, z = runs
    dx = x.writeCheckpoint(str(tmp_path / "bg" / "chk00002"), background=True)
    x.run_steps(2)
    x.checkpoint_wait()
    dy = y.writeCheckpoint(str(tmp_path / "sync" / "chk00002"))
    z.run_steps(2)
    compare_single(x, z)
    assert x.nstep == 4 and not os.path.exists(dx + ".temp")
    names = sorted(os.path.relpath(os.path.join(r, f), dx) for r, _, fs in os.walk(dx) for f in fs)
    assert names == sorted(os.path.relpath(os.path.join(r, f), dy) for r, _, fs in os.walk(dy) for f in fs)
    assert "Level_0/SD_0_New_MF_D_00000" in names and "Header" in names and "CPUtime" in names
    for f in names:
        if f == "CPUtime":
            for d in (dx, dy):
                s = open(os.path.join(d, f)).read()
                assert s == "%.17g" % float(s)
            continue
        assert filecmp.cmp(os.path.join(dx, f), os.path.join(dy, f), shallow=False), f
    from castro_amd.checkpoint import read_checkpoint
    ck = read_checkpoint(dx)
    assert ck["nstep"] == 2 and ck["time"] == y.time
    assert np.array_equal(ck["levels"][0]["state"][0].view(np.int64), y.S_new().cpu().numpy().view(np.int64))
    b = ck["levels"][0]["headers"][0][0]
    S = y.S_new()
    assert b["min"] == [float(S[n].min()) for n in range(8)] and b["max"] == [float(S[n].max()) for n in range(8)]


def test_background_write_with_tracers(hydro, tmp_path):
    """writeCheckpoint(background=True) of a run with tracers, the next steps issued at once: the steps advect the particle
    arrays in place while the checkpoint is on its way, so the checkpoint must hold a snapshot taken on the stepping stream.
    The Particles files equal those of a synchronous checkpoint of an identical run, the restarted run equals the run that
    never stopped; then the same through evolve with check_int"""
    import castro_amd
    pos = np.random.default_rng(1301).uniform(0.05, 0.95, size=(20000, 3))
    make = lambda **kw: castro_amd.Castro((32, 32, 32), hydro=hydro, params=castro_amd.default_params(init_shrink=1.0),
                                          tracers=castro_amd.TracerParticles(positions=pos), **kw)
    runs = []
    for _ in range(3):
        c = make()
        _init(c)
        for _ in range(3):
            c.step()
        runs.append(c)
    a, x, y = runs
    dx = x.writeCheckpoint(str(tmp_path / "bg" / "chk00003"), background=True)
    for c in (x, a):
        for _ in range(3):
            c.step()
    x.checkpoint_wait()
    dy = y.writeCheckpoint(str(tmp_path / "sync" / "chk00003"))
    assert not torch.equal(x.tracers.pos, y.tracers.pos), "the particles must have moved while the checkpoint was written"
    for f in ("Particles/DATA_00000", "Particles/Header", "Level_0/SD_0_New_MF_D_00000", "Level_0/SD_0_New_MF_H", "Header"):
        assert filecmp.cmp(os.path.join(dx, f), os.path.join(dy, f), shallow=False), f
    r = make()
    r.restart(dx)
    for _ in range(3):
        r.step()
    compare_single(a, r)
    compare_single(a, x)
    # evolve with check_int: a background checkpoint after steps 2 and 4, the steps going on at once
    e = make(check_int=2, check_file=str(tmp_path / "ev"))
    _init(e)
    e.evolve(1.0, max_step=6)
    e.close()
    compare_single(a, e)
    r = make()
    r.restart(str(tmp_path / "ev00004"))
    r.step(), r.step()
    compare_single(a, r)

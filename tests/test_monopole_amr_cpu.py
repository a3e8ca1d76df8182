"""Monopole gravity on AMR levels without a GPU: the exported symbols of both builds, the refusals, the per-level n1d, the time
branch of make_radial_gravity, the level combination, and CastroAmr(gravity=MonopoleGravity(...)) on the numpy restatement
(tests/monopole_amr_ref.py) -- a uniform sphere against the analytic field, the dust collapse on one and two ranks, three levels."""
import ctypes as C
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import monopole_amr_ref as A
from tests import monopole_ref as R

NEW_SYMBOLS = ("castro_amd_radial_mass_mf_ex", "castro_amd_radial_combine", "castro_amd_grav_bc_fill_fab", "castro_amd_sources_mf_g")
_CACHE = {}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_both_builds_export_the_new_symbols_and_structs():
    from castro_amd import _lib
    import __graft_entry__ as g
    if not all(os.path.exists(_lib.lib_path(m)) for m in _lib.NUMERICS_MODES):
        g.build()
    for mode in _lib.NUMERICS_MODES:
        lib = _lib.load(mode)
        for name in NEW_SYMBOLS:
            assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, (mode, name)
        assert lib.castro_amd_abi_version() == 5
    # castro_amd_radial_box: 2 x int[3], two fabs of 40 bytes, a pointer, two doubles
    assert C.sizeof(_lib.RadialBox) == 24 + 2 * 40 + 8 + 16
    assert [f for f, _ in _lib.RadialBox._fields_] == ["lo", "hi", "state_old", "state_new", "mask", "omalpha", "alpha"]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "castro_hydro_amd.h")).read()
    assert "castro_amd_radial_box" in hdr and "#define CASTRO_AMD_ABI_VERSION 5" in hdr


def test_refusals_and_the_new_form(oracle):
    import castro_amd
    P = oracle.default_params()
    mk = lambda: A.MonopoleAmrOracleBackend()
    patch = ((4, 4, 4), (11, 11, 11))
    with pytest.raises(NotImplementedError, match="make_radial_gravity"):            # the bare string keeps its refusal
        castro_amd.CastroAmr((16, 16, 16), patch_crse=patch, do_grav=True, gravity_type="monopole")
    with pytest.raises(NotImplementedError, match="diffusion"):
        castro_amd.CastroAmr((16, 16, 16), patch_crse=patch, params=P, make_hydro=mk, do_grav=True,
                             gravity=castro_amd.MonopoleGravity(), diffusion=castro_amd.make_diffusion(1.0))
    with pytest.raises(ValueError, match="periodic"):
        castro_amd.CastroAmr((16, 16, 16), patch_crse=patch, params=P, make_hydro=mk, do_grav=True, lo_bc=(0, 0, 0), hi_bc=(0, 0, 0),
                             gravity=castro_amd.MonopoleGravity())
    with pytest.raises(NotImplementedError, match="periodic"):
        castro_amd.CastroAmr((16, 16, 16), patch_crse=patch, params=P, make_hydro=mk, do_grav=True, lo_bc=(0, 2, 2), hi_bc=(0, 2, 2),
                             gravity=castro_amd.MonopoleGravity())
    with pytest.raises(ValueError, match="at least 1"):
        castro_amd.MonopoleGravity(drdxfac=0)
    with pytest.raises(ValueError, match="drdxfac <= 5"):
        castro_amd.CastroAmr((16, 16, 16), patch_crse=patch, params=P, make_hydro=mk, do_grav=True, gravity=castro_amd.MonopoleGravity(drdxfac=6))
    with pytest.raises(ValueError, match="do_grav"):
        castro_amd.CastroAmr((16, 16, 16), patch_crse=patch, params=P, make_hydro=mk, gravity=castro_amd.MonopoleGravity())
    with pytest.raises(TypeError):
        castro_amd.CastroAmr((16, 16, 16), patch_crse=patch, params=P, make_hydro=mk, do_grav=True, gravity="monopole")
    a = castro_amd.CastroAmr((16, 16, 16), patch_crse=patch, params=P, make_hydro=mk, do_grav=True, gravity=castro_amd.MonopoleGravity(drdxfac=5))
    assert all(b.monopole and b.grav_old.shape == (3, 18, 18, 18) for lev in a.lev for b in lev.boxes)


def test_n1d_per_level(oracle):
    import castro_amd
    g = castro_amd.MonopoleGravity(drdxfac=2)
    castro_amd.CastroAmr((24, 20, 16), patches=[((2, 2, 2), (9, 9, 9)), ((6, 6, 6), (17, 17, 17))], params=oracle.default_params(),
                         make_hydro=lambda: A.MonopoleAmrOracleBackend(), do_grav=True, gravity=g, prob_hi=(3.0, 2.5, 2.0))
    # drdxfac * (int(sqrt(nx^2 + ny^2 + nz^2)) + 8) of the level's domain: sqrt(1232) = 35.1, sqrt(4928) = 70.2, sqrt(19712) = 140.4
    assert [g.n1d(l) for l in range(3)] == [2 * (35 + 8), 2 * (70 + 8), 2 * (140 + 8)]
    assert g.n1d(1) != 2 * g.n1d(0) and g.params(2).n1d == 296 and g.params(1).drdxfac == 2
    assert g.params(1).max_radius_all_in_domain == 1.0                   # probhi - centre of the domain, level-independent


def test_time_branch():
    from castro_amd.gravity import time_branch
    t0, t1 = 1.0, 1.5
    assert time_branch(t0, t0, t1) == ("old", 0.0)
    assert time_branch(t1, t0, t1) == ("new", 1.0)
    assert time_branch(t0 + 0.4e-6 * (t1 - t0), t0, t1)[0] == "old" and time_branch(t1 - 0.4e-6 * (t1 - t0), t0, t1)[0] == "new"
    kind, alpha = time_branch(1.25, t0, t1)
    assert kind == "interp" and alpha == (1.25 - t0) / (t1 - t0) == 0.5
    assert time_branch(1.1, t0, t1) == ("interp", (1.1 - t0) / (t1 - t0))
    assert time_branch(2.0, 2.0, 2.0) == ("new", 1.0)                    # eps == 0: the new data
    for bad in (0.9, 1.6):
        with pytest.raises(RuntimeError, match="make_radial_gravity"):
            time_branch(bad, t0, t1)


def test_interpolated_binning_is_made_on_the_interpolated_density():
    from castro_amd import _lib
    geom = _lib.make_geom((8, 8, 8))
    mono = _lib.make_monopole((8, 8, 8), geom, (0.0, 0.0, 0.0), 2)
    rng = np.random.default_rng(2)
    ro, rn = rng.uniform(1.0, 2.0, (8, 8, 8)), rng.uniform(1.0, 2.0, (8, 8, 8))
    ro[0, 0, 0], rn[0, 0, 0] = 1.0, -7.0 / 3.0                            # (1 * 0.7) + (-7/3 * 0.3) rounds to 0 or not: as computed
    ref = A.radial_mass_ex([(ro, rn, (0, 0, 0), None, 0.7, 0.3)], geom, mono)
    same = R.radial_mass([((ro * 0.7) + (rn * 0.3), (0, 0, 0), None)], geom, mono)
    assert np.array_equal(ref["mass"], same["mass"]) and np.array_equal(ref["count"], same["count"])
    one = A.radial_mass_ex([(ro, rn, (0, 0, 0), None, 1.0, 0.0)], geom, mono)
    assert np.array_equal(one["mass"], R.radial_mass([(ro, (0, 0, 0), None)], geom, mono)["mass"])


def test_combination_conserves_mass():
    """no bin is cut off when n1d of every level is the exact multiple: the combined sum is the sum of the level sums"""
    rng = np.random.default_rng(4)
    n1ds = [32, 64, 128]
    arrs = [(np.ldexp(rng.integers(1, 2 ** 20, n).astype(np.float64), -10), np.ldexp(rng.integers(1, 2 ** 20, n).astype(np.float64), -12))
            for n in n1ds]                                                   # dyadic values: every sum below is exact
    for level in (1, 2):
        m, v = A.combine(arrs, n1ds, level)
        assert m.sum() == sum(a[0].sum() for a in arrs[:level + 1]) and v.sum() == sum(a[1].sum() for a in arrs[:level + 1])
        assert m[5] == arrs[level][0][5] + sum(arrs[l][0][5 >> (level - l)] / 2 ** (level - l) for l in range(level - 1, -1, -1))
    # a non-multiple n1d: the bins beyond ratio * (n1d / ratio) receive nothing from the coarser level
    n2 = [43, 78]
    a2 = [(np.ones(43), np.ones(43)), (np.zeros(78), np.zeros(78))]
    m, _ = A.combine(a2, n2, 1)
    assert np.all(m == 0.5) and len(m) == 78
    n3 = [43, 79]
    m, _ = A.combine([a2[0], (np.zeros(79), np.zeros(79))], n3, 1)
    assert np.all(m[:78] == 0.5) and m[78] == 0.0
    with pytest.raises(AssertionError):
        A.combine([(np.ones(30), np.ones(30)), (np.zeros(78), np.zeros(78))], [30, 78], 1)


def test_uniform_sphere_follows_the_analytic_field_on_both_levels(oracle):
    """rho = rho_0 inside r_0, the octant on base 16^3 with a fixed 16^3 fine patch at the centre: g(r) = -(4/3) pi G rho_0 r inside
    the sphere on both levels, and a sibling-free ghost zone of the fine level holds the interpolated coarse value"""
    import castro_amd
    rho_0, r_0 = 1.0e3, 0.5
    g = castro_amd.MonopoleGravity(drdxfac=2, center=(0.0, 0.0, 0.0))
    a = castro_amd.CastroAmr((16, 16, 16), patch_crse=((0, 0, 0), (7, 7, 7)), params=oracle.default_params(),
                             make_hydro=lambda: A.MonopoleAmrOracleBackend(), do_grav=True, gravity=g, lo_bc=(3, 3, 3), hi_bc=(2, 2, 2))
    for l, lev in enumerate(a.lev):
        b = lev.boxes[0]
        x = [(np.arange(b.lo[d], b.hi[d] + 1) + 0.5) * b.geom.dx[d] for d in range(3)]
        Z, Y, X = np.meshgrid(x[2], x[1], x[0], indexing="ij")
        rho = np.where(np.sqrt(X * X + Y * Y + Z * Z) < r_0, rho_0, 1.e-6 * rho_0)
        for S in (b.S_new(), b.S_old_b[:, 4:-4, 4:-4, 4:-4]):
            S.zero_()
            S[0] = torch.from_numpy(rho)
            S[4] = S[5] = 1.0
        lev.t_old, lev.t_new, lev.alpha = 0.0, 1.0 / 2 ** l, 0.0
    for l in (0, 1):
        g.get_new_grav_vector(l, time=1.0, a=1.0)          # level 1 at the coarse new time: the coarse level's new data and grav_new
        b = a.lev[l].boxes[0]
        gv = b.grav_new.numpy()
        x = [(np.arange(b.gravbox[0][d], b.gravbox[1][d] + 1) + 0.5) * b.geom.dx[d] for d in range(3)]
        Z, Y, X = np.meshgrid(x[2], x[1], x[0], indexing="ij")
        r = np.sqrt(X * X + Y * Y + Z * Z)
        want = -(4.0 / 3.0) * math.pi * g.Gconst * rho_0 * r
        inner = (r > 2.0 * b.geom.dx[0]) & (r < 0.8 * r_0) & (X > 0) & (Y > 0) & (Z > 0)
        mag = -np.sqrt(gv[0] ** 2 + gv[1] ** 2 + gv[2] ** 2)
        err = np.abs(mag[inner] - want[inner]).max() / np.abs(want[inner]).max()
        print("uniform sphere, level %d: max deviation from the analytic field %.3g" % (l, err))
        assert err < 0.05 and np.all(gv[0][inner] < 0.0)
        # symmetry faces: the ghost zone mirrors the first zone inside, normal component negated
        assert np.array_equal(gv[0][1:-1, 1:-1, 0], -gv[0][1:-1, 1:-1, 1]) and np.array_equal(gv[1][1:-1, 1:-1, 0], gv[1][1:-1, 1:-1, 1])
    # the fine level's upper ghost zones lie inside the domain under the coarse level only: cell_cons_interp of the coarse data
    fb, cb = a.lev[1].boxes[0], a.lev[0].boxes[0]
    ghost = fb.grav_new.numpy()[0][5, 5, -1]
    direct = fb.grav_new.numpy()[0][5, 5, -2]
    assert ghost < 0.0 and abs(ghost - direct) < 0.2 * abs(direct)
    m, v, go, gn = g.radial_gravity(1)
    assert m.shape == (g.n1d(1),) and np.all(gn[:20] < 0.0)


def test_a_sibling_ghost_zone_carries_the_siblings_bits():
    """interpolate_monopole_grav is a function of the index alone: the ghost zone of a box over a sibling's valid zone holds the
    sibling's bits, so the Gravity_Type FillPatch needs no copy there"""
    from castro_amd import _lib
    geom = _lib.make_geom((16, 16, 16))
    mono = _lib.make_monopole((16, 16, 16), geom, (0.5, 0.5, 0.5), 2)
    rg = -np.linspace(0.1, 3.0, mono.n1d) ** 1.5
    b1, b2 = ((0, 0, 0), (7, 15, 15)), ((8, 0, 0), (15, 15, 15))
    out = []
    for bx in (b1, b2):
        gb = (tuple(x - 1 for x in bx[0]), tuple(x + 1 for x in bx[1]))
        gv = np.zeros((3,) + tuple(gb[1][d] - gb[0][d] + 1 for d in (2, 1, 0)))
        R.interpolate(rg, geom, mono, gv, gb)
        out.append(gv)
    assert np.array_equal(out[0][:, :, :, -1].view(np.int64), out[1][:, :, :, 1].view(np.int64))       # x = 8: ghost of b1, valid of b2
    assert np.array_equal(out[1][:, :, :, 0].view(np.int64), out[0][:, :, :, -2].view(np.int64))       # x = 7


def _dust(oracle):
    if "dust" not in _CACHE:
        ref, dts, s = A.dust_amr_sensitivity(oracle)
        _CACHE["dust"] = (ref, dts, s)
    return _CACHE["dust"]


def test_dust_collapse_amr_one_rank(oracle):
    """2 coarse steps = 4 fine advances: the coarse level enters with its old, its interpolated and its new data; gravity points
    inwards on both levels and the run differs from the gravity-free one by far more than the tolerance"""
    ref, dts, s = _dust(oracle)
    print("AMR dust collapse: deviation per field and level for one ulp per bin in the radial masses, s =", s)
    seen = []
    keep = ref.gravity._bin_level
    ref.gravity._bin_level = lambda *a: (seen.append((a[0], a[1], keep(*a))), seen[-1][2])[1]
    ref.step()
    ref.gravity._bin_level = keep
    coarse_for_fine = [b for l, level, b in seen if level == 1 and l == 0]
    assert coarse_for_fine == ["old", "interp", "interp", "new"], coarse_for_fine
    free, _ = A.dust_amr_run(lambda: A.MonopoleAmrOracleBackend(), oracle.default_params(**R.DUST_PARAMS), do_grav=False, steps=3)
    for l, (x, y) in enumerate(zip(A.level_states(ref), A.level_states(free))):
        tol = np.maximum(1e-10, 100.0 * s[l])
        d = R.field_deviation(x, y)
        assert d[R.UMX] > 1e4 * tol[R.UMX], (l, d, tol)
        assert np.all(s[l] < 1e-8)
        m, v, go, gn = ref.gravity.radial_gravity(l)
        dr = ref.lev[l].geom.dx[0] / A.AMR_DRDXFAC
        rc = (np.arange(ref.gravity.n1d(l)) + 0.5) * dr
        inside = rc < 0.9 * R.DUST_PROB["r_0"]
        assert np.all(gn[inside] < 0.0) and np.all(np.diff(gn[inside]) < 0.0), l
        b = ref.lev[l].boxes[0]
        gv = b.grav_new.numpy()
        assert np.all(gv[:, 1:-1, 1:-1, 1:-1][:, 2:6, 2:6, 2:6] < 0.0), "the octant's gravity points to the corner at the centre"


def _worker(rank, world, port, out_path):
    import torch.distributed as dist
    import castro_amd
    from oracle import oracle_lib as O
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        a, dts = A.dust_amr_run(lambda: A.MonopoleAmrOracleBackend(), O.default_params(**R.DUST_PARAMS), comm=castro_amd.DistComm())
        levels = [a.gather_level(l) for l in range(len(a.lev))]
        if rank == 0:
            np.savez(out_path, dts=np.array(dts), **{"S%d" % l: lv[0][1] for l, lv in enumerate(levels)},
                     grav=a.gravity.radial_gravity(1)[3])
    finally:
        dist.destroy_process_group()


def test_two_ranks_agree_with_one_within_the_summation_tolerance(tmp_path, oracle):
    """The hierarchy on two gloo ranks (level 0 on rank 0, the fine box on rank 1) against one.  The boxes of a level are binned
    where they live and the level's array is summed over the ranks: with one box per level the sums have the same terms in the
    same order.  Tolerance per field as everywhere: max(1e-10, 100 s)."""
    out = str(tmp_path / "dist.npz")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = np.load(out)
    ref, dts, s = _dust(oracle)
    want, wdts = _CACHE.get("two") or (None, None)
    if want is None:
        r2, wdts = A.dust_amr_run(lambda: A.MonopoleAmrOracleBackend(), oracle.default_params(**R.DUST_PARAMS))
        want = A.level_states(r2)
        _CACHE["two"] = (want, wdts)
    for l in range(2):
        tol = np.maximum(1e-10, 100.0 * s[l])
        d = R.field_deviation(got["S%d" % l], want[l])
        print("two ranks against one, level %d: deviation per field" % l, d, "tolerance", tol)
        assert np.all(d <= tol), (l, d, tol)
    assert np.allclose(got["dts"], np.array(wdts), rtol=1e-12, atol=0.0)


def test_three_levels_one_coarse_step(oracle):
    """ratio 4 between level 0 and level 2 and n1d values that are no multiples of each other: 70, 126, 236"""
    a, dts = A.dust_amr_run(lambda: A.MonopoleAmrOracleBackend(), oracle.default_params(**R.DUST_PARAMS), steps=1,
                            patches=[((0, 0, 0), (7, 7, 7)), ((0, 0, 0), (7, 7, 7))])
    g = a.gravity
    assert [g.n1d(l) for l in range(3)] == [70, 126, 236] and g.n1d(2) // 4 <= g.n1d(0)
    assert dts[0] > 0.0
    m2, v2, go2, gn2 = g.radial_gravity(2)
    # the combined mass of the finest level is the mass of the sphere: (4/3) pi r_0^3 rho_0 to the accuracy of the zone averages
    want = 4.0 / 3.0 * math.pi * R.DUST_PROB["r_0"] ** 3 * R.DUST_PROB["rho_0"]
    assert abs(m2.sum() - want) < 0.02 * want, (m2.sum(), want)
    assert np.all(gn2[:100] < 0.0)
    for lev in a.lev:
        assert np.isfinite(lev.boxes[0].S_new().numpy()).all()


def test_refine_tagging_runs_through_a_regrid(oracle):
    """CastroAmr(refine=..., gravity=MonopoleGravity(...)): the fine level follows the density tags; with regrid_int = 2 the third
    coarse step regrids (the tags of a collapse this young give the boxes it had), a dropped fine level is rebuilt by regrid(0)
    with fresh gravity FABs, tables and masks, and the gravity of both levels is constructed again"""
    import castro_amd
    g = castro_amd.MonopoleGravity(drdxfac=2, center=(0.0, 0.0, 0.0))
    a = castro_amd.CastroAmr((16, 16, 16), params=oracle.default_params(**R.DUST_PARAMS), make_hydro=lambda: A.MonopoleAmrOracleBackend(),
                             do_grav=True, gravity=g, refine=[("density", "value_greater", 5.e8)], regrid_int=2, max_level=1,
                             blocking_factor=8, **R.DUST_GEOM)
    a.initData("dust_collapse", **R.DUST_PROB)
    assert len(a.lev) == 2
    dts = [a.step() for _ in range(3)]
    assert all(d > 0.0 for d in dts) and a.level_count[0] == 1, "the third step went through Amr::regrid"
    before = g.radial_gravity(1)[3]
    assert np.all(before[1:40] < 0.0)
    a._drop_fine()
    assert 1 not in g._lev and g._lev[0]["tables"] == {}
    assert a.regrid(0) and len(a.lev) == 2
    fb = a.lev[1].boxes[0]
    assert fb.grav_new.abs().max() == 0.0, "a rebuilt level starts with empty Gravity_Type data"
    a.lev[1].t_old, a.lev[1].t_new, a.lev[1].alpha = a.time, a.time, 1.0
    g.get_new_grav_vector(1, time=a.time, a=1.0)
    assert fb.grav_new.abs().max() > 0.0 and np.isfinite(fb.grav_new.numpy()).all()


def test_single_level_and_level_zero_are_one_route(oracle):
    """grav_source_type = 2 reads no ghost zone of the field: Castro(gravity_type="monopole") and a CastroAmr with no refined
    level agree bit for bit after two steps"""
    A.assert_routes_agree_inside(*A.single_and_hierarchy(lambda: A.MonopoleAmrOracleBackend(), oracle.default_params(**R.DUST_PARAMS),
                                                         grav_source_type=2))

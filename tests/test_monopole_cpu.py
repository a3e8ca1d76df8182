"""CPU tests of monopole self-gravity (gravity.gravity_type = MonopoleGrav): the numpy restatement (tests/monopole_ref.py) against
the analytic field of a uniform sphere and against mass conservation, the C ABI additions in both builds, the refusals, the
set-up arithmetic of the driver, and the driver on one and on two gloo ranks with the restatement as the backend."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import monopole_ref as R
from tests.test_driver_cpu import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _uniform_deviation(n, drdxfac):
    """the largest relative deviation of radial_grav from -(4/3) pi G rho rc over the bins whose centre lies between a quarter
    of max_radius_all_in_domain and max_radius_all_in_domain, for rho = 1 on the whole unit cube of n^3 zones about its middle"""
    from castro_amd import _lib
    geom = _lib.make_geom((n, n, n))
    mono = _lib.make_monopole((n, n, n), geom, (0.5, 0.5, 0.5), drdxfac)
    ref = R.radial_mass([(np.ones((n, n, n)), (0, 0, 0), None)], geom, mono)
    assert ref["dropped"] == 0
    g = R.radial_gravity(ref["mass"], ref["vol"], geom, mono)
    dr = geom.dx[0] / drdxfac
    rc = (np.arange(mono.n1d) + 0.5) * dr
    sel = (rc >= 0.25 * mono.max_radius_all_in_domain) & (rc < mono.max_radius_all_in_domain)
    exact = -(4.0 / 3.0) * math.pi * mono.Gconst * 1.0 * rc
    return float(np.abs(g[sel] / exact[sel] - 1.0).max())


def test_uniform_density_follows_the_analytic_field_and_converges_with_drdxfac():
    """Uniform density over the whole domain: radial_grav[i] = -(4/3) pi G rho rc but for the deviation of the binned volumes from
    the analytic shells.  The restatement's values (the prototype's, printed below; nothing fixed in advance):
        16^3: drdxfac 1: 1.266e-01, drdxfac 4: 1.713e-02        32^3: drdxfac 1: 5.042e-02, drdxfac 4: 5.085e-03
    Asserted: the deviation shrinks with drdxfac at either size, and with the resolution at either drdxfac."""
    dev = {(n, f): _uniform_deviation(n, f) for n in (16, 32) for f in (1, 4)}
    for k in sorted(dev):
        print("uniform sphere %d^3 drdxfac %d: max relative deviation %.3e" % (k[0], k[1], dev[k]))
    for n in (16, 32):
        assert dev[(n, 4)] < dev[(n, 1)]
    for f in (1, 4):
        assert dev[(32, f)] < dev[(16, f)]


@pytest.mark.parametrize("center,drdxfac", [((0.5, 0.5, 0.5), 1), ((0.5, 0.5, 0.5), 4), ((0.0, 0.0, 0.0), 2)])
def test_mass_is_conserved_when_no_subzone_is_dropped(center, drdxfac):
    """sum(radial_mass) == octant_factor * sum(rho * vol) within the summation bound: every sub-zone lands in a bin (n1d of the
    domain reaches past its farthest corner), so the histogram only regroups the terms"""
    from castro_amd import _lib
    n = (12, 10, 8)
    geom = _lib.make_geom(n)
    mono = _lib.make_monopole(n, geom, center, drdxfac)
    rho = np.random.default_rng(5).uniform(0.5, 2.0, size=n[::-1])
    ref = R.radial_mass([(rho, (0, 0, 0), None)], geom, mono)
    assert ref["dropped"] == 0 and int(ref["count"].sum()) == rho.size * drdxfac ** 3
    octant = 8.0 if center == (0.0, 0.0, 0.0) else 1.0
    assert R.octant_factor(geom, mono) == octant
    vol = geom.dx[0] * geom.dx[1] * geom.dx[2]
    total = math.fsum((rho * vol).ravel().tolist())
    nterms = rho.size * drdxfac ** 3
    got = math.fsum(ref["mass"].tolist())
    # the terms vol_frac * rho and rho * vol differ by a few roundings each: 4 ulps per term on top of the two exact sums
    assert abs(got - octant * total) <= (4 * 2.0 ** -52 + nterms * 2.0 ** -52) * octant * total
    assert np.array_equal(ref["vol"], ref["count"] * R.vol_frac(geom, mono))


def test_new_symbols_and_struct_exist_in_both_builds():
    from castro_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "castro_hydro_amd.h")).read()
    names = ("castro_amd_radial_mass_mf", "castro_amd_radial_gravity", "castro_amd_monopole_grav_fab",
             "castro_amd_old_gravity_source_gfab", "castro_amd_new_gravity_source_gfab")
    for p in (_lib.lib_path("exact"), _lib.lib_path("contract")):
        if not os.path.exists(p):
            import __graft_entry__ as g
            g.build()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS
        for mode in _lib.NUMERICS_MODES:
            assert getattr(_lib.load(mode), name) is not None, (mode, name)
    assert "typedef struct castro_amd_monopole_params" in hdr
    assert re.search(r"#define CASTRO_AMD_ABI_VERSION 5\b", hdr)
    # int n1d, drdxfac; double center[3], max_radius_all_in_domain, Gconst
    assert C.sizeof(_lib.MonopoleParams) == 2 * 4 + 5 * 8
    assert _lib.GCONST == 6.67428e-8


def test_n1d_and_max_radius_of_a_24x20x16_domain():
    """n1d = drdxfac * (int(sqrt(24^2 + 20^2 + 16^2)) + 2 * 4) = drdxfac * (int(35.09...) + 8) = 43 drdxfac;
    max_radius_all_in_domain = min(3 - 1, 2.5 - 1, 2 - 0.5) = 1.5 for prob_hi (3, 2.5, 2) and the centre (1, 1, 0.5)"""
    from castro_amd import _lib
    n = (24, 20, 16)
    geom = _lib.make_geom(n, prob_hi=(3.0, 2.5, 2.0))
    assert 35 * 35 <= 24 * 24 + 20 * 20 + 16 * 16 < 36 * 36
    for f in (1, 2, 4):
        m = _lib.make_monopole(n, geom, (1.0, 1.0, 0.5), f)
        assert m.n1d == 43 * f and m.drdxfac == f
        assert m.max_radius_all_in_domain == 1.5
        assert m.Gconst == 6.67428e-8
    assert _lib.monopole_max_drdxfac((0.1, 0.1, 0.1)) == 5            # 12 * 5 + 3 = 63 <= 64 < 12 * 6 + 3


def test_refusals(oracle):
    import castro_amd
    hyd = R.MonopoleOracleBackend()
    kw = dict(params=oracle.default_params(), hydro=hyd, do_grav=True, gravity_type="monopole")
    with pytest.raises(NotImplementedError, match="make_radial_gravity"):
        castro_amd.CastroAmr((16, 16, 16), patch_crse=((4, 4, 4), (11, 11, 11)), do_grav=True, gravity_type="monopole")
    with pytest.raises(ValueError, match="periodic"):
        castro_amd.Castro((16, 16, 16), lo_bc=(0, 0, 0), hi_bc=(0, 0, 0), **kw)
    with pytest.raises(ValueError, match="at least 1"):
        castro_amd.Castro((16, 16, 16), drdxfac=0, **kw)
    with pytest.raises(ValueError, match="drdxfac <= 5"):
        castro_amd.Castro((16, 16, 16), drdxfac=6, **kw)
    with pytest.raises(ValueError, match="gravity_type"):
        castro_amd.Castro((16, 16, 16), params=oracle.default_params(), hydro=hyd, do_grav=True, gravity_type="poisson")
    c = castro_amd.Castro((16, 16, 16), drdxfac=5, **kw)                # the limit itself is taken
    assert c.n1d == 5 * (27 + 8) and c.monopole
    # constant gravity is what every existing call gets
    assert castro_amd.Castro((16, 16, 16), params=oracle.default_params(), hydro=hyd, do_grav=True, const_grav=-1.0).monopole is False


def test_dust_collapse_driver_one_rank(oracle):
    """the driver on the restatement: gravity points inwards and grows monotonically inside r_0, the run differs from the same
    run without gravity, and radial_gravity() returns what the last construction left"""
    ref, dts, s = R.dust_sensitivity(oracle)
    print("dust collapse: deviation per field for one ulp per bin in the radial masses, s =", s)
    mass, vol, grav = ref.radial_gravity()
    assert mass.shape == vol.shape == grav.shape == (ref.n1d,)
    dr = ref.geom.dx[0] / R.DUST_DRDXFAC
    rc = (np.arange(ref.n1d) + 0.5) * dr
    inside = rc < 0.9 * R.DUST_PROB["r_0"]
    assert np.all(grav[inside] < 0.0) and np.all(np.diff(grav[inside]) < 0.0)
    free, fdts = R.dust_collapse_run(R.MonopoleOracleBackend(), oracle.default_params(**R.DUST_PARAMS), do_grav=False)
    tol = np.maximum(1e-10, 100.0 * s)
    d = R.field_deviation(ref.S_new().numpy(), free.S_new().numpy())
    assert d[R.UMX] > 1e4 * tol[R.UMX], (d, tol)
    assert np.all(s < 1e-8)


def _worker(rank, world, port, out_path):
    import torch.distributed as dist
    import castro_amd
    from oracle import oracle_lib as O
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c, dts = R.dust_collapse_run(R.MonopoleOracleBackend(), O.default_params(**R.DUST_PARAMS), comm=castro_amd.DistComm())
        mine = c.S_new().contiguous()
        parts = [torch.zeros_like(mine) for _ in range(world)] if rank == 0 else None
        dist.gather(mine, parts, dst=0)
        boxes = [None] * world
        dist.all_gather_object(boxes, (c.lo, c.hi))
        if rank == 0:
            n = R.DUST_N
            full = np.zeros((8, n[2], n[1], n[0]))
            for p, (lo, hi) in zip(parts, boxes):
                full[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = p.numpy()
            np.savez(out_path, S=full, dts=np.array(dts), grav=c.radial_gravity()[2])
    finally:
        dist.destroy_process_group()


def test_two_ranks_agree_with_one_within_the_summation_tolerance(tmp_path, oracle):
    """Dust collapse on two gloo ranks against one.  Not bitwise: each rank bins its own box and the allreduce adds the two
    partial masses of a bin, another order of the same terms.  Tolerance per field: max(1e-10, 100 * s) of the field's max, s
    the deviation of a run whose radial masses differ by one ulp per bin; the time steps agree to 1e-12 relative."""
    out = str(tmp_path / "dist.npz")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = np.load(out)
    ref, dts, s = R.dust_sensitivity(oracle)
    tol = np.maximum(1e-10, 100.0 * s)
    d = R.field_deviation(got["S"], ref.S_new().numpy())
    print("two ranks against one: deviation per field", d, "tolerance", tol, "s", s)
    assert np.all(d <= tol), (d, tol)
    assert np.allclose(got["dts"], np.array(dts), rtol=1e-12, atol=0.0)
    g1 = ref.radial_gravity()[2]
    assert np.abs(got["grav"] - g1).max() <= 1e-12 * np.abs(g1).max()


def test_out_of_domain_ghost_zone_keeps_the_interpolation(oracle):
    """grav_source_type = 4 reads the ghost zone of grav_new: on a single level it holds the interpolated value"""
    from tests import monopole_amr_ref as A
    c, _ = R.dust_collapse_run(R.MonopoleOracleBackend(), oracle.default_params(**R.DUST_PARAMS), steps=1)
    assert c.grav_source_type == 4
    A.assert_ghost_zone_is_the_interpolation(c, exact=True)

"""CPU tests of explicit thermal diffusion (castro.diffuse_temp = 1): the numpy restatement of the term against a case worked
by hand, the C ABI additions, and the driver logic of castro_amd.Castro -- old / new source stages, the ghost fill of S_new in
front of the new-time term, the diffusion limit on the time step, castro.do_hydro = 0 -- with the oracle's clean_state and the
numpy term as the backend (tests/diffusion_ref.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import diffusion_ref as R
from tests.test_driver_cpu import _free_port


class _G:
    """the fields of castro_amd_geom the restatement reads"""

    def __init__(self, dx, domlo, domhi, lo_bc, hi_bc, coord=0):
        self.dx, self.domlo, self.domhi, self.lo_bc, self.hi_bc, self.coord = dx, domlo, domhi, lo_bc, hi_bc, coord


def test_restatement_against_a_hand_computed_zone():
    """One zone (1,1,1) with its six neighbours; cutoff 1, cutoff_hi 3, conductivity 2, scale 0.5, dx = (0.5, 0.25, 1):
      k_cc: centre rho 2 -> 0.5 * (2 * 0.5) = 0.5;  east rho 3 (not below cutoff_hi) -> 1.0;  west rho 5 -> 1.0 (unused);
            south rho 1 (not above the cutoff) -> 0;  north rho 2.5 -> 0.5 * (2 * 0.75) = 0.75;  below rho 2 -> 0.5;  top rho 4 -> 1.0
      x: the low face is the physical boundary (outflow, i = domlo): 0;  high face 0.75 * (14 - 10) = 3      -> fx = 3
      y: low 0.25 * (10 - 6) = 1;  high 0.625 * (12 - 10) = 1.25                                            -> fy = 0.25
      z: low 0.5 * (10 - 9) = 0.5;  high 0.75 * (8 - 10) = -1.5                                             -> fz = -2
      DiffTerm = 4 * 3 + 16 * 0.25 + 1 * (-2) = 14,   A = 4 * 3 + 16 * 2.25 + 1 * 2 = 50"""
    from castro_amd import _lib
    U = np.zeros((8, 3, 3, 3))
    U[R.URHO] = 7.0
    U[R.UTEMP] = np.nan                                   # corners and edges are never read
    rho, T = U[R.URHO], U[R.UTEMP]
    rho[1, 1, 1], T[1, 1, 1] = 2.0, 10.0
    rho[1, 1, 0], T[1, 1, 0] = 5.0, 100.0                 # behind the physical boundary: whatever it holds
    rho[1, 1, 2], T[1, 1, 2] = 3.0, 14.0
    rho[1, 0, 1], T[1, 0, 1] = 1.0, 6.0
    rho[1, 2, 1], T[1, 2, 1] = 2.5, 12.0
    rho[0, 1, 1], T[0, 1, 1] = 2.0, 9.0
    rho[2, 1, 1], T[2, 1, 1] = 4.0, 8.0
    diff = _lib.make_diffusion(2.0, 1.0, 3.0, 0.5)
    g = _G((0.5, 0.25, 1.0), (1, -8, -8), (8, 8, 8), (2, 0, 0), (2, 0, 0))
    D, A = R.diffusion_term(U, ((0, 0, 0), (2, 2, 2)), (1, 1, 1), (1, 1, 1), g, diff)
    assert D.shape == (1, 1, 1) and D[0, 0, 0] == 14.0 and A[0, 0, 0] == 50.0
    # the ghost zone behind the boundary may hold anything, a NaN included
    T[1, 1, 0] = np.nan
    D2, _ = R.diffusion_term(U, ((0, 0, 0), (2, 2, 2)), (1, 1, 1), (1, 1, 1), g, diff)
    assert D2[0, 0, 0] == 14.0
    # with the face inside the domain the west neighbour counts: 0.75 * (10 - 100) = -67.5 -> fx = 70.5
    T[1, 1, 0] = 100.0
    g.domlo = (0, -8, -8)
    D3, _ = R.diffusion_term(U, ((0, 0, 0), (2, 2, 2)), (1, 1, 1), (1, 1, 1), g, diff)
    assert D3[0, 0, 0] == 4.0 * 70.5 + 16.0 * 0.25 - 2.0
    assert not R.supported(_G(g.dx, g.domlo, g.domhi, (1, 0, 0), (2, 0, 0))) and not R.supported(_G(g.dx, g.domlo, g.domhi, (2, 0, 0), (2, 3, 0)))


def test_diffusion_struct_and_symbols_in_both_builds():
    from castro_amd import _lib
    assert C.sizeof(_lib.Diffusion) == 4 * 8
    assert C.sizeof(_lib.DiffusionBox) == 2 * 12 + 2 * C.sizeof(_lib.Fab)
    d = _lib.make_diffusion(10.0)
    assert (d.const_conductivity, d.diffuse_cutoff_density, d.diffuse_cutoff_density_hi, d.diffuse_cond_scale_fac) == (10.0, -1e200, -1e200, 1.0)
    names = ("castro_amd_temp_diffusion_fab", "castro_amd_temp_diffusion_mf", "castro_amd_estdt_temp_diffusion_fab",
             "castro_amd_estdt_temp_diffusion_mf", "castro_amd_sources_mf_ex")
    for p in (_lib.lib_path("exact"), _lib.lib_path("contract")):
        if not os.path.exists(p):
            import __graft_entry__ as g
            g.build()
    for mode in _lib.NUMERICS_MODES:
        L = _lib.load(mode)
        for name in names:
            assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None, (mode, name)


def test_amr_refuses_diffusion():
    import castro_amd
    with pytest.raises(NotImplementedError, match="single level"):
        castro_amd.CastroAmr((16, 16, 16), patch_crse=((4, 4, 4), (11, 11, 11)), diffusion=castro_amd.make_diffusion(1.0))


def _diffusion_test_run(n, oracle, stop_time=1.e-3):
    import castro_amd
    params = oracle.default_params(cfl=0.3, init_shrink=0.1, change_max=1.1)
    c = castro_amd.Castro((n, n, n), params=params, hydro=R.DiffusionOracleBackend(), do_hydro=False,
                          diffusion=castro_amd.make_diffusion(const_conductivity=10.0))
    c.initData("diffusion_test")
    e0 = c.S_new()[R.UEDEN].numpy().copy()
    c.evolve(stop_time)
    assert abs(c.time - stop_time) <= 1e-15 and c.dt_limiter == "diffusion"
    T = c.S_new()[R.UTEMP].numpy()
    err = float(np.abs(T - c.diffusion_test_analytic(c.time)).max())
    return c, err, e0


# L-infinity error of Temp against the analytic Gaussian at t = 1e-3, from a numpy prototype of this scheme that evolves T directly
PROTOTYPE_ERR = {32: 1.402e-2, 64: 3.99e-3}


def test_diffusion_test_converges_to_the_analytic_gaussian(oracle):
    """Exec/unit_tests/diffusion_test with castro.do_hydro = 0, outflow boundaries, cfl = 0.3 (the inputs file's 0.5 is outside
    the stability interval of the predictor-corrector in 3-D): second order, each error within 2 % of the prototype's, and the
    total energy conserved (zero boundary flux, and the two sides of a face compute the same product)."""
    errs = {}
    for n in (32, 64):
        c, err, e0 = _diffusion_test_run(n, oracle)
        errs[n] = err
        print("diffusion_test %d^3: %d steps, Linf(Temp) = %.6e (prototype %.4e)" % (n, c.nstep, err, PROTOTYPE_ERR[n]))
        e1 = c.S_new()[R.UEDEN].numpy()
        drift = abs(float(e1.sum()) - float(e0.sum()))
        print("diffusion_test %d^3: |sum rhoE change| / sum |rhoE| = %.3e" % (n, drift / float(np.abs(e0).sum())))
        assert drift <= 1e-10 * float(np.abs(e0).sum())
        assert float(np.abs(c.S_new()[1:4].numpy()).max()) == 0.0            # nothing moves
    for n in (32, 64):
        assert abs(errs[n] - PROTOTYPE_ERR[n]) <= 0.02 * PROTOTYPE_ERR[n], (n, errs[n])
    assert errs[32] / errs[64] > 3.0


# ---- two gloo ranks against one: the ghost fill of S_new in front of the new-time term -------------------------------------
SEDOV_N, SEDOV_STEPS, SEDOV_COND = (32, 32, 32), 5, 1.e10


def _sedov_diffusion(comm, hydro, params):
    import castro_amd
    c = castro_amd.Castro(SEDOV_N, params=params, hydro=hydro, comm=comm, diffusion=castro_amd.make_diffusion(SEDOV_COND))
    c.initData("sedov", r_init=0.12, nsub=3)
    dts, lim = [], []
    for _ in range(SEDOV_STEPS):
        dts.append(c.step())
        lim.append(c.dt_limiter)
    return c, dts, lim


def _worker(rank, world, port, out_path):
    import torch.distributed as dist
    import castro_amd
    from oracle import oracle_lib as O
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c, dts, lim = _sedov_diffusion(castro_amd.DistComm(), R.DiffusionOracleBackend(), O.default_params())
        mine = c.S_new().contiguous()
        parts = [torch.zeros_like(mine) for _ in range(world)] if rank == 0 else None
        dist.gather(mine, parts, dst=0)
        boxes = [None] * world
        dist.all_gather_object(boxes, (c.lo, c.hi))
        if rank == 0:
            n = SEDOV_N
            full = np.zeros((8, n[2], n[1], n[0]))
            for p, (lo, hi) in zip(parts, boxes):
                full[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = p.numpy()
            np.savez(out_path, S=full, dts=np.array(dts), lim=np.array(lim))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_diffusion_are_bitwise_identical_to_one(tmp_path, oracle):
    """Sedov 32^3 with hydro and a conductivity large enough for the diffusion limit to set the time step: the new-time term
    reads T of S_new one zone outside the box, so two ranks equal one only if S_new is ghost-filled in front of it."""
    out = str(tmp_path / "dist.npz")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = np.load(out)
    from castro_amd.castro import SingleComm
    c, dts, lim = _sedov_diffusion(SingleComm(), R.DiffusionOracleBackend(), oracle.default_params())
    assert "diffusion" in lim and list(got["lim"]) == lim
    assert np.array_equal(got["dts"], np.array(dts))
    assert np.array_equal(got["S"], c.S_new().numpy())
    # the term did something: the same run without diffusion ends elsewhere
    import castro_amd
    from tests.oracle_backend import OracleBackend
    p = castro_amd.Castro(SEDOV_N, params=oracle.default_params(), hydro=OracleBackend())
    p.initData("sedov", r_init=0.12, nsub=3)
    p.step()
    assert p.dt > dts[0]

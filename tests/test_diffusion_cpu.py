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


# ---- the restatement against a manufactured solution -----------------------------------------------------------------------
# T = a x^2 + b y^2 + c z^2 + p x + q y + r z + s at the zone centres of an anisotropic index space that does not start at zero.
# The second difference of a quadratic is exact, so with a constant conductivity k every direction contributes 2 k a away from
# a physical face; on a Neumann face the flux through the face is dropped and the normal part is the one-sided difference
#   low face:  k (T+ - T0) / dx^2 =  k (a (2 x0 + dx) + p) / dx,      high face:  -k (T0 - T-) / dx^2 = -k (a (2 x0 - dx) + p) / dx
# Nothing here is taken from the restatement: a dh on the wrong axis or the wrong side of a face is an O(1) error.
MS_N, MS_DOMLO = (70, 9, 40), (-5, 3, 100)
MS_PROB_LO, MS_PROB_HI = (0.0, -1.0, 2.0), (1.4, -0.1, 2.5)
MS_K, MS_QUAD, MS_LIN, MS_CONST = 3.0, (1.3, -0.7, 2.1), (0.4, -1.1, 0.6), 5.0
# the issue's boundaries (x periodic: four physical faces), and a mixed pair in x -- outflow low, interior high: each side is a
# flag of its own in the operator -- for a fifth
MS_BCS = {"periodic-x": ((0, 2, 4), (0, 2, 2)), "outflow-low-x": ((2, 2, 4), (0, 2, 2))}


def _manufactured(lo_bc, hi_bc):
    n, g = MS_N, 1
    dx = tuple((MS_PROB_HI[d] - MS_PROB_LO[d]) / n[d] for d in range(3))
    domhi = tuple(MS_DOMLO[d] + n[d] - 1 for d in range(3))
    geom = _G(dx, MS_DOMLO, domhi, lo_bc, hi_bc)
    x = [MS_PROB_LO[d] + (np.arange(-g, n[d] + g) + 0.5) * dx[d] for d in range(3)]            # ghost zones included
    X, Y, Z = x[0][None, None, :], x[1][None, :, None], x[2][:, None, None]
    T = (MS_QUAD[0] * X * X + MS_QUAD[1] * Y * Y + MS_QUAD[2] * Z * Z + MS_LIN[0] * X + MS_LIN[1] * Y + MS_LIN[2] * Z + MS_CONST)
    box = R.grow(MS_DOMLO, domhi, g)
    U = np.zeros((8,) + R.shape_of(box))
    U[R.URHO], U[R.UTEMP] = 1.0, T
    # the closed form, direction by direction
    part = []
    for d in range(3):
        xc = x[d][g:-g]
        e = np.full(n[d], 2.0 * MS_K * MS_QUAD[d])
        if lo_bc[d] != 0:
            e[0] = MS_K * (MS_QUAD[d] * (2.0 * xc[0] + dx[d]) + MS_LIN[d]) / dx[d]
        if hi_bc[d] != 0:
            e[-1] = -MS_K * (MS_QUAD[d] * (2.0 * xc[-1] - dx[d]) + MS_LIN[d]) / dx[d]
        shape = [1, 1, 1]
        shape[2 - d] = n[d]
        part.append(e.reshape(shape))
    want = part[0] + part[1] + part[2]
    # the inputs are polynomials rounded to double: every T carries eps / 2 |T|, a face difference eps max|T|, six of them per
    # zone weighted k / dx_d^2, the products, the sums and the closed form's own rounding on top -- 16 eps k max|T| sum_d 1 / dx_d^2
    tol = 16.0 * np.finfo(float).eps * MS_K * float(np.abs(T).max()) * sum(1.0 / (h * h) for h in dx)
    return geom, U, box, domhi, want, tol


@pytest.mark.parametrize("bcs", sorted(MS_BCS))
def test_restatement_against_a_manufactured_solution(bcs):
    from castro_amd import _lib
    lo_bc, hi_bc = MS_BCS[bcs]
    geom, U, box, domhi, want, tol = _manufactured(lo_bc, hi_bc)
    D, A = R.diffusion_term(U, box, MS_DOMLO, domhi, geom, _lib.make_diffusion(MS_K))
    assert D.shape == MS_N[::-1] and tol < 1e-8
    inner = tuple(slice(1 if lo_bc[d] != 0 else 0, -1 if hi_bc[d] != 0 else None) for d in (2, 1, 0))
    err = float(np.abs(D[inner] - 2.0 * MS_K * sum(MS_QUAD)).max())
    print("%s: away from the physical faces max |D - %.17g| = %.3e (bound %.3e)" % (bcs, 2.0 * MS_K * sum(MS_QUAD), err, tol))
    assert abs(2.0 * MS_K * sum(MS_QUAD) - 16.2) < 1e-14 and np.array_equal(want[inner], np.full_like(D[inner], 2.0 * MS_K * sum(MS_QUAD)))
    assert err <= tol
    faces = 0
    for d in range(3):
        for side, bc in ((0, lo_bc[d]), (-1, hi_bc[d])):
            if bc == 0:
                continue
            idx = [slice(None)] * 3
            idx[2 - d] = side
            idx = tuple(idx)
            w = np.broadcast_to(want, D.shape)[idx]
            ferr = float(np.abs(D[idx] - w).max())
            print("%s: %s face of direction %d max |D - closed form| = %.3e" % (bcs, "high" if side else "low", d, ferr))
            assert ferr <= tol, (d, side)
            assert float(np.abs(w - 2.0 * MS_K * sum(MS_QUAD)).min()) > 1.0          # the one-sided form is nowhere near the interior's
            faces += 1
    assert faces == (4 if bcs == "periodic-x" else 5)
    assert float(np.abs(D - want).max()) <= tol                                     # edges and corners: two and three faces at once
    assert (A >= np.abs(D) * (1.0 - 1e-12)).all()                                    # the scale of the face contributions


def test_restatement_constant_temperature_gives_an_exact_zero():
    """densities across the ramp (below the cutoff, on it, above cutoff_hi) under a constant T: every face difference is an exact
    zero whatever the face conductivity, so the term and its scale A are 0.0 in every zone, physical faces included"""
    from castro_amd import _lib
    lo_bc, hi_bc = MS_BCS["periodic-x"]
    geom, U, box, domhi, _, _ = _manufactured(lo_bc, hi_bc)
    rng = np.random.default_rng(11)
    U[R.URHO] = rng.uniform(0.5, 3.5, size=U[R.URHO].shape)
    U[R.UTEMP] = 1.75
    rho = U[R.URHO]
    assert (rho <= 1.0).mean() > 0.1 and ((rho > 1.0) & (rho < 2.5)).mean() > 0.3 and (rho >= 2.5).mean() > 0.2
    D, A = R.diffusion_term(U, box, MS_DOMLO, domhi, geom, _lib.make_diffusion(MS_K, 1.0, 2.5, 0.7))
    assert np.array_equal(D, np.zeros_like(D)) and np.array_equal(A, np.zeros_like(A))


def test_unit_test_inputs():
    """the input helpers of the GPU tests: the periodic image, NaN behind a physical face, neighbour data at an interior edge"""
    rng = np.random.default_rng(3)
    lo, hi, g = (-5, 3, 100), (-5, 5, 103), 2                       # one zone wide in x
    geom = _G((1.0, 1.0, 1.0), (-5, 3, 90), (-5, 5, 103), (0, 2, 4), (0, 2, 2))
    U, box = R.ghosted_state(rng, lo, hi, g, geom)
    assert box == ((-7, 1, 98), (-3, 7, 105)) and U.shape == (8, 8, 7, 5)
    v = U[:, g:-g, g:-g, g:-g]
    assert np.isfinite(v).all()
    for i in range(5):                                            # every x ghost zone is the image of the single valid column
        assert np.array_equal(U[:, g:-g, g:-g, i:i + 1], v)
    assert np.isnan(U[:, :, :g]).all() and np.isnan(U[:, :, -g:]).all()            # y: both faces physical
    assert np.isnan(U[:, -g:]).all() and np.isfinite(U[:, :g, g:-g]).all()       # z: high face physical, low edge interior
    assert R.region(box, lo, hi) == (slice(2, 6), slice(2, 5), slice(2, 3))
    # the stage restatement: zero outside [lo, hi] and outside the two energies, and S_new = S_old + dt * source
    U[np.isnan(U)] = 1.0
    from castro_amd import _lib
    diff = _lib.make_diffusion(3.0, 1.0, 2.5, 0.7)
    sbox = R.grow(lo, hi, 3)
    src, Sn, A = R.source_stage(0, U, box, np.full_like(U, -3.0), box, sbox, 7, lo, hi, geom, diff, 0.25)
    D, A0 = R.diffusion_term(U, box, lo, hi, geom, diff)
    sv = R.region(sbox, lo, hi)
    assert np.array_equal(src[R.UEDEN][sv], D) and np.array_equal(src[R.UEINT][sv], D) and np.array_equal(A, A0)
    src[R.UEDEN][sv] = src[R.UEINT][sv] = 0.0
    assert not src.any()
    assert np.array_equal(Sn[R.UEDEN][g:-g, g:-g, g:-g], v[R.UEDEN] + 0.25 * D) and np.array_equal(Sn[R.URHO][g:-g, g:-g, g:-g], v[R.URHO])
    assert (Sn[:, :g] == -3.0).all() and (Sn[:, :, :, -g:] == -3.0).all()
    # stage 1 with S_new = S_old: 0.5 D - 0.5 D is an exact zero
    src1, Sn1, A1 = R.source_stage(1, U, box, U, box, (lo, hi), 7, lo, hi, geom, diff, 0.25)
    assert not src1.any() and np.array_equal(Sn1, U) and np.array_equal(A1, 0.5 * A0 + 0.5 * A0)


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

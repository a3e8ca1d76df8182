"""CPU tests of Poisson gravity: the numpy restatement (tests/poisson_ref.py) against the recorded values of the reference's own
Legendre functions and multipole_add (tests/golden/stub_probe/multipole_vectors.npz), against known answers and a dense solve,
and the driver castro_amd.Castro(do_grav=True, poisson=PoissonGravity(...)) on PoissonOracleBackend.

Three tests here check the restatement alone -- test_dense_check, test_level_passes_known_answers and
test_grad_phi_of_a_linear_potential -- and so need nothing of the product: they validate the reference the GPU tests compare the
kernels with (the dense check is the one the solver's tests rest on).  Every other test needs the package's Poisson interface."""
import os

import numpy as np
import pytest

from tests import poisson_ref as R
from tests import monopole_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U52 = 2.0 ** -52
SHAPES = [(16, 16, 16), (16, 8, 12), (6, 10, 14), (5, 7, 9)]          # four, three, two and one level
DX = (0.11, 0.13, 0.09)
FOURPIG = 4.0 * np.pi * 6.67428e-8
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the restatement against the reference's own functions -----------------------------------------------------------------------
@pytest.mark.parametrize("lnum", [0, 2, 6])
def test_restatement_reproduces_the_probe(lnum):
    """Legendre and associated Legendre values bit for bit: the recurrences are pure arithmetic, and the one pow of P_m^m is taken
    from the C library the probe was linked with (assoc_step(libm=True): numpy's vectorised pow differs from it in the last bit
    for some zones).  The vectorised path the device comparisons use stays within its allowance of those values.  The terms of
    multipole_add (pow, cos, sin of numpy against the C library's) within the per-term allowance of poisson_ref."""
    V = np.load(os.path.join(ROOT, "tests", "golden", "stub_probe", "multipole_vectors.npz"))
    Z = V["zones"]
    cosT, phiA, r, rho, vol = (Z[:, n].copy() for n in range(5))
    assert (np.abs(cosT) == 1.0).sum() >= 3 and (phiA == 0.0).any() and (phiA == np.pi).any() and (cosT == 0.0).any()
    n1 = lnum + 1
    st = [None, None, None]
    for l in range(n1):
        R.leg_step(l, st, cosT)
        assert np.array_equal(_bits(st[0]), _bits(V["l%d.leg" % lnum][:, l])), l
    worst_a = 0.0
    for m in range(1, n1):
        st, err, sl = [None, None, None], [None, None, None], [None, None, None]
        for l in range(m, n1):
            R.assoc_step(l, m, st, cosT, err)
            R.assoc_step(l, m, sl, cosT, libm=True)
            want = V["l%d.assoc" % lnum][:, l, m]
            assert np.array_equal(_bits(sl[0]), _bits(want)), (l, m, int((_bits(sl[0]) != _bits(want)).sum()))
            d = np.abs(st[0] - want)
            worst_a = max(worst_a, float((d[err[0] > 0] / err[0][err[0] > 0]).max()) if (err[0] > 0).any() else 0.0)
            assert np.all(d <= err[0]), (l, m)
            assert np.all(st[0][np.abs(cosT) == 1.0] == 0.0), "P_l^m vanishes on the axis"
    terms = R.zone_terms(lnum, cosT, phiA, r, rho, vol)
    worst = 0.0
    for (kind, l, m), (t, dt) in terms.items():
        want = V["l%d.%s" % (lnum, ("qL0", "qLC", "qLS")[kind])]
        want = want[:, l] if kind == 0 else want[:, l, m]
        d = np.abs(t - want)
        assert np.all(d <= dt), (kind, l, m, d.max(), dt.max())
        if (dt > 0).any():
            worst = max(worst, float((d[dt > 0] / dt[dt > 0]).max()))
    # every entry the loop nest does not reach is zero in the recording
    for kind, name in ((1, "qLC"), (2, "qLS")):
        W = V["l%d.%s" % (lnum, name)]
        for l in range(n1):
            for m in range(n1):
                if (kind, l, m) not in terms:
                    assert np.all(W[:, l, m] == 0.0)
    print("lnum %d: worst deviation / allowance: associated Legendre through numpy's pow %.3g, terms %.3g" % (lnum, worst_a, worst))


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def _geom(n, prob_hi=(1.0, 1.0, 1.0), lo_bc=(2, 2, 2), hi_bc=(2, 2, 2)):
    from castro_amd import _lib
    return _lib.make_geom(n, prob_hi=prob_hi, lo_bc=lo_bc, hi_bc=hi_bc)


def test_moment_of_a_single_zone_at_the_centre():
    """lnum = 0, one zone whose centre is the centre: r = 0, pow(0, 0) = 1, P_0 = 1: qL0(0) = rho * (V / rmax^3), the two products
    of the restatement -- one term, nothing to sum"""
    from castro_amd import _lib
    n = (5, 5, 5)
    geom = _geom(n, prob_hi=(1.0, 1.5, 2.0))
    center = tuple(geom.problo[d] + 2.5 * geom.dx[d] for d in range(3))
    mp = _lib.make_multipole(geom, center, 0)
    assert mp.rmax == 0.5 * 2.0 * np.sqrt(3.0)
    rho = np.zeros((1, 1, 1))
    rho[0, 0, 0] = 3.7e5
    q, bound = R.moments([(rho, (2, 2, 2), None)], geom, mp)
    V = geom.dx[0] * geom.dx[1] * geom.dx[2]
    assert q.shape == (3,) and q[0] == 3.7e5 * (V * (1.0 / (mp.rmax * mp.rmax * mp.rmax))) and q[1] == 0.0 and q[2] == 0.0
    assert abs(q[0] - 3.7e5 * V / mp.rmax ** 3) <= 4.0 * U52 * q[0]


def test_boundary_potential_of_a_single_dense_zone():
    """lnum = 0 and one zone of mass m = rho V at a distance d from a ghost point: phi = -G m / d.  Roundings between the two
    sides (each at most 2^-53 relative; the coordinates before the division by rmax are common to both): the restatement takes
    rmax^3 twice (2 + 2), its inverse (1), V (2), V / rmax^3 (1), rho * that (1), the three coordinates / rmax (3, which move r
    by at most 1.5 roundings after the squares, sums and the root: count 3 + 3), pow(r, -1) (1), two products (2), -G * (1),
    / rmax (1): 23; the known answer takes V (2), rho V (1), d (3), G m (1), / d (1): 8.  31 * 2^-53 < 16 * 2^-52."""
    from castro_amd import _lib
    n = (6, 4, 8)
    geom = _geom(n, prob_hi=(1.5, 1.0, 2.0))
    zone = (3, 1, 5)
    center = tuple(geom.problo[d] + (zone[d] + 0.5) * geom.dx[d] for d in range(3))
    mp = _lib.make_multipole(geom, center, 0)
    rho = np.zeros((n[2], n[1], n[0]))
    rho[zone[2], zone[1], zone[0]] = 2.5e7
    q, _ = R.moments([(rho, (0, 0, 0), None)], geom, mp)
    box = ((-1, -1, -1), tuple(n))
    SENT = 777.0
    phi = np.full((n[2] + 2, n[1] + 2, n[0] + 2), SENT)
    outside, _ = R.phi_bc(q, geom, mp, phi, box)
    assert np.all(phi[~outside] == SENT) and np.all(phi[outside] != SENT), "only the ghost shell is written"
    assert outside.sum() == phi.size - n[0] * n[1] * n[2]
    m = 2.5e7 * (geom.dx[0] * geom.dx[1] * geom.dx[2])
    loc = []
    for d in range(3):
        i = np.arange(-1, n[d] + 1)
        x = np.where(i > n[d] - 1, geom.problo[d] + i * geom.dx[d], np.where(i < 0, geom.problo[d] + (i + 1.0) * geom.dx[d],
                                                                              geom.problo[d] + (i + 0.5) * geom.dx[d])) - center[d]
        sh = [1, 1, 1]
        sh[2 - d] = n[d] + 2
        loc.append(x.reshape(sh))
    dist = np.sqrt(loc[0] ** 2 + loc[1] ** 2 + loc[2] ** 2) + np.zeros(phi.shape)
    with np.errstate(divide="ignore"):
        want = -mp.Gconst * m / dist           # the zone itself is at distance 0: a valid zone, not compared
    rel = np.abs(phi[outside] - want[outside]) / np.abs(want[outside])
    print("single dense zone: worst relative deviation from -G m / d = %.3g ulp" % (rel.max() / U52))
    assert rel.max() <= 16.0 * U52


def test_a_ghost_zone_on_the_centre_has_phi_exactly_zero():
    """the centre on the high corner of the domain: the corner ghost zone sits on the faces in all three directions, its
    coordinates are problo + n dx - probhi = 0 exactly, r = 0 < 1e-12 and phi = 0 -- not the NaN of 0 / 0"""
    from castro_amd import _lib
    n = (8, 8, 8)
    geom = _geom(n)
    mp = _lib.make_multipole(geom, (1.0, 1.0, 1.0), 2)
    rng = np.random.default_rng(5)
    q, _ = R.moments([(rng.uniform(1.0, 2.0, size=(8, 8, 8)), (0, 0, 0), None)], geom, mp)
    phi = np.full((10, 10, 10), np.nan)
    R.phi_bc(q, geom, mp, phi, ((-1, -1, -1), (8, 8, 8)))
    assert phi[9, 9, 9] == 0.0 and not np.signbit(phi[9, 9, 9])
    shell = np.ones(phi.shape, dtype=bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.isfinite(phi[shell]).all() and (phi[shell] != 0.0).sum() == shell.sum() - 1


# ---- multigrid -------------------------------------------------------------------------------------------------------------------
def _mg_case(n):
    """a right-hand side of one sign with a dense clump (as 4 pi G rho is) and boundary values of a point mass, on zones of
    three different widths"""
    if n not in _CACHE:
        rng = np.random.default_rng(sum(n))
        shape = (n[2], n[1], n[0])
        rho = rng.uniform(1.0e3, 2.0e3, size=shape)
        rho[n[2] // 2, n[1] // 3, n[0] // 2] = 5.0e6
        phi = np.zeros((n[2] + 2, n[1] + 2, n[0] + 2))
        k, j, i = np.meshgrid(*[np.arange(-1, m + 1) for m in shape], indexing="ij")
        d = np.sqrt(((i - n[0] / 2 + 0.5) * DX[0]) ** 2 + ((j - n[1] / 3 + 0.5) * DX[1]) ** 2 + ((k - n[2] / 2 + 0.5) * DX[2]) ** 2)
        shell = np.ones(phi.shape, dtype=bool)
        shell[1:-1, 1:-1, 1:-1] = False
        phi[shell] = (-6.67428e-8 * 5.0e6 * DX[0] * DX[1] * DX[2] / np.maximum(d, DX[2]))[shell]
        _CACHE[n] = (rho, phi)
    rho, phi = _CACHE[n]
    return rho.copy(), phi.copy()


def independent_residual(n, phi, b):
    """b - lap(phi) written another way: the ghost zones are filled with 2 g - p first, then the plain 7-point stencil"""
    G = phi.copy()
    G[1:-1, 1:-1, 0] = 2.0 * phi[1:-1, 1:-1, 0] - phi[1:-1, 1:-1, 1]
    G[1:-1, 1:-1, -1] = 2.0 * phi[1:-1, 1:-1, -1] - phi[1:-1, 1:-1, -2]
    G[1:-1, 0, 1:-1] = 2.0 * phi[1:-1, 0, 1:-1] - phi[1:-1, 1, 1:-1]
    G[1:-1, -1, 1:-1] = 2.0 * phi[1:-1, -1, 1:-1] - phi[1:-1, -2, 1:-1]
    G[0, 1:-1, 1:-1] = 2.0 * phi[0, 1:-1, 1:-1] - phi[1, 1:-1, 1:-1]
    G[-1, 1:-1, 1:-1] = 2.0 * phi[-1, 1:-1, 1:-1] - phi[-2, 1:-1, 1:-1]
    c = G[1:-1, 1:-1, 1:-1]
    lap = ((G[1:-1, 1:-1, 2:] - 2.0 * c + G[1:-1, 1:-1, :-2]) / DX[0] ** 2 + (G[1:-1, 2:, 1:-1] - 2.0 * c + G[1:-1, :-2, 1:-1]) / DX[1] ** 2
           + (G[2:, 1:-1, 1:-1] - 2.0 * c + G[:-2, 1:-1, 1:-1]) / DX[2] ** 2)
    return b - lap


def solved(n):
    key = ("solved", n)
    if key not in _CACHE:
        rho, phi = _mg_case(n)
        out = R.solve(n, DX, phi, rho, FOURPIG)
        _CACHE[key] = (rho, phi, out)
    return _CACHE[key]


@pytest.mark.parametrize("n,nlev", list(zip(SHAPES, (4, 3, 2, 1))))
def test_vcycles_meet_the_stopping_rule(n, nlev):
    from castro_amd import _lib
    assert len(R.levels(n, DX)) == nlev == len(_lib.poisson_level_extents(n))
    assert [L.n for L in R.levels(n, DX)] == _lib.poisson_level_extents(n)
    rho, phi, (cycles, ok, rnorm, hist) = solved(n)
    b = FOURPIG * rho
    tol = R.stopping_tolerance(b)
    print("%s: %d levels, %d cycles, norms %s, tolerance %.3g" % (n, nlev, cycles, ["%.3g" % h for h in hist[2:]], tol))
    assert ok and 1 <= cycles <= 40 and rnorm <= tol and len(hist) == cycles + 3
    assert hist[0] == np.abs(b).max() and hist[1] == b.max()
    assert np.all(np.diff(hist[2:]) < 0.0), "every cycle lowers the residual"
    ind = np.abs(independent_residual(n, phi, b)).max()
    # the stopping rule itself, plus what two orders of the same sum can differ by: each formulation makes fewer than 8 roundings
    # per zone, each at most 2^-53 of the sum of the magnitudes of the zone's terms (mag: cx (|xm| + |xp| + |2 p|) + ... + |b|)
    mag = np.zeros(R.levels(n, DX)[0].shape)
    R.residual(R.levels(n, DX)[0], phi, b, mag)
    assert ind <= tol + 8.0 * U52 * mag.max(), (ind, tol, mag.max())


def test_dense_check():
    """(16, 8, 12), 1536 unknowns: phi against numpy.linalg.solve of the assembled operator,
    ||phi - phi_dense|| <= ||A^-1|| (||r|| + ||r_dense|| + gamma), every term computed (poisson_ref.dense_check)"""
    n = (16, 8, 12)
    rho, phi, _ = solved(n)
    L = R.levels(n, DX)[0]
    A = R.dense_operator(L)
    b = FOURPIG * rho
    # the assembled operator is the residual's: b - (A phi + boundary part) == residual, to rounding
    x = phi[1:-1, 1:-1, 1:-1].reshape(-1)
    r_mat = (b - R.boundary_rhs(L, phi)).reshape(-1) - A @ x
    r_ref = R.residual(L, phi, b).reshape(-1)
    assert np.abs(r_mat - r_ref).max() <= 64.0 * U52 * (np.abs(A) @ np.abs(x)).max()
    dev, bound = R.dense_check(L, phi, b)
    print("dense check (16, 8, 12): deviation %.3g, bound %.3g" % (dev, bound))
    assert dev <= bound


def test_level_passes_known_answers():
    """restriction of a constant is the constant, prolongation adds the coarse value to its eight children, the smoother leaves
    an exact solution of the discrete equations where it is (to rounding), the residual of phi = 0 is b"""
    n = (16, 8, 12)
    lev = R.levels(n, DX)
    assert np.all(R.restrict(np.full(lev[0].shape, 3.25)) == 3.25)
    pc = np.zeros(lev[1].gshape)
    pc[1:-1, 1:-1, 1:-1] = np.arange(np.prod(lev[1].shape), dtype=np.float64).reshape(lev[1].shape)
    pf = np.ones(lev[0].gshape)
    R.prolong(pc, pf)
    assert pf[1, 1, 1] == 1.0 and pf[2, 2, 2] == 1.0 and pf[3, 1, 1] == 1.0 + pc[2, 1, 1] and np.all(pf[0] == 1.0)
    rho, phi, _ = solved(n)
    b = FOURPIG * rho
    assert np.array_equal(R.residual(lev[0], np.zeros(lev[0].gshape), b), b)
    before = phi.copy()
    R.smooth(lev[0], phi, b, 0)
    R.smooth(lev[0], phi, b, 1)
    assert np.abs(phi - before).max() <= 1e-8 * np.abs(before).max()
    assert R.norm(np.array([[-3.0, 2.0]])) == (3.0, 2.0) and np.isnan(R.norm(np.array([1.0, np.nan]))[0])


def test_grad_phi_of_a_linear_potential():
    """phi = a . x, the ghost zones holding the face values: every face gradient is exact up to rounding, g = -a everywhere"""
    n = (6, 5, 4)
    a = (0.5, -0.25, 2.0)
    k, j, i = np.meshgrid(*[np.arange(-1, m + 1, dtype=np.float64) for m in (n[2], n[1], n[0])], indexing="ij")
    pos = []
    for idx, m, h in ((i, n[0], DX[0]), (j, n[1], DX[1]), (k, n[2], DX[2])):
        pos.append(np.where(idx < 0, 0.0, np.where(idx > m - 1, m * h, (idx + 0.5) * h)))
    phi = a[0] * pos[0] + a[1] * pos[1] + a[2] * pos[2]
    g = R.grad_phi(phi, DX)
    for d in range(3):
        assert np.abs(g[d] + a[d]).max() <= 1e-13 * abs(a[d])


# ---- driver ----------------------------------------------------------------------------------------------------------------------
def _kw(oracle, **over):
    kw = dict(params=oracle.default_params(), hydro=R.PoissonOracleBackend(), do_grav=True)
    kw.update(over)
    return kw


def test_refusals(oracle):
    import castro_amd
    from castro_amd import _lib
    from castro_amd.castro import SingleComm
    PG = castro_amd.PoissonGravity
    n = (16, 16, 16)
    # the string keeps its two values: the feature is selected by the keyword alone
    with pytest.raises(ValueError, match="gravity_type"):
        castro_amd.Castro(n, gravity_type="poisson", **_kw(oracle))
    with pytest.raises(NotImplementedError, match="periodic"):
        castro_amd.Castro(n, lo_bc=(0, 2, 2), hi_bc=(0, 2, 2), poisson=PG(), **_kw(oracle))
    with pytest.raises(NotImplementedError, match="Symmetry"):
        castro_amd.Castro(n, lo_bc=(3, 3, 3), poisson=PG(), **_kw(oracle))

    class TwoRanks(SingleComm):
        size = 2
    with pytest.raises(NotImplementedError, match="more than one rank"):
        castro_amd.Castro(n, comm=TwoRanks(), poisson=PG(), **_kw(oracle))
    with pytest.raises(ValueError, match="monopole"):
        castro_amd.Castro(n, gravity_type="monopole", poisson=PG(), **_kw(oracle))
    with pytest.raises(ValueError, match="monopole"):
        castro_amd.Castro(n, gravity=castro_amd.MonopoleGravity(), box=((4, 4, 4), (11, 11, 11)), poisson=PG(), **_kw(oracle))
    with pytest.raises(ValueError, match="do_grav"):
        castro_amd.Castro(n, poisson=PG(), **_kw(oracle, do_grav=False))
    with pytest.raises(ValueError, match="HSE"):
        castro_amd.Castro(n, lo_bc=(2, 2, 1), ext_bc=_lib.make_ext_bc(zl="hse"), poisson=PG(), **_kw(oracle))
    with pytest.raises(NotImplementedError, match="use_point_mass"):
        castro_amd.Castro(n, use_point_mass=True, point_mass=1.0, poisson=PG(), **_kw(oracle))
    with pytest.raises(NotImplementedError, match="single level"):
        castro_amd.CastroAmr(n, patch_crse=((4, 4, 4), (11, 11, 11)), do_grav=True, poisson=PG())
    with pytest.raises(NotImplementedError, match="refined patch"):
        castro_amd.Castro(n, box=((4, 4, 4), (11, 11, 11)), poisson=PG(), **_kw(oracle))
    with pytest.raises(NotImplementedError, match="check_int"):
        castro_amd.Castro(n, check_int=5, poisson=PG(), **_kw(oracle))
    with pytest.raises(NotImplementedError, match="no multipole_moments_mf"):
        castro_amd.Castro(n, poisson=PG(), **_kw(oracle, hydro=MR.MonopoleOracleBackend()))
    with pytest.raises(ValueError, match="max_multipole_order"):
        PG(max_multipole_order=_lib.MAX_MULTIPOLE + 1)
    with pytest.raises(ValueError, match="max_multipole_order"):
        PG(max_multipole_order=-1)
    with pytest.raises(ValueError, match=r"n_cell = \(250, 250, 250\)"):
        castro_amd.Castro((250, 250, 250), alloc=False, poisson=PG(), **_kw(oracle))       # refused before any array is made
    c = castro_amd.Castro(n, poisson=PG(max_multipole_order=_lib.MAX_MULTIPOLE), **_kw(oracle))       # the cap itself is taken
    assert c.poisson is not None and c.grav_fab and not c.monopole and not c.host_free_ok()
    with pytest.raises(NotImplementedError, match="writeCheckpoint"):
        c.writeCheckpoint("/nonexistent/chk")
    with pytest.raises(NotImplementedError, match="restart"):
        c.restart("/nonexistent/chk")
    with pytest.raises(ValueError, match="one Castro"):
        castro_amd.Castro(n, poisson=c.poisson, **_kw(oracle))
    assert c.poisson.plan is not None
    c.close()                                                    # gives the multigrid plan back; idempotent
    assert c.poisson.plan is None
    c.close()
    # every existing call is what it was
    plain = castro_amd.Castro(n, **_kw(oracle, const_grav=-1.0))
    assert plain.poisson is None and plain.grav_fab is False
    with pytest.raises(RuntimeError, match="poisson="):
        plain.phi_grav()


def _dust(oracle):
    if "dust" not in _CACHE:
        ref, dts, s = R.dust_sensitivity(oracle)
        free, _ = R.dust_collapse_run(R.PoissonOracleBackend(), oracle.default_params(**R.DUST_PARAMS), do_grav=False)
        _CACHE["dust"] = (ref, dts, s, free)
    return _CACHE["dust"]


def test_dust_collapse_driver(oracle):
    """16^3, the full star, 3 steps: gravity points inwards at every zone inside r_0, the run differs from the same run without
    gravity, and the warm-started new-time solve takes fewer cycles than the first solve of the run"""
    ref, dts, s, free = _dust(oracle)
    print("dust collapse with Poisson gravity: s per field =", s, "dts", dts)
    g = ref.grav_new.numpy()[:, 1:-1, 1:-1, 1:-1]
    x = [(np.arange(16) + 0.5) * ref.geom.dx[d] - R.DUST_CENTER[d] for d in range(3)]
    X, Y, Z = x[0][None, None, :], x[1][None, :, None], x[2][:, None, None]
    rr = np.sqrt(X * X + Y * Y + Z * Z)
    g_r = (g[0] * X + g[1] * Y + g[2] * Z) / rr
    inside = rr < R.DUST_PROB["r_0"]
    assert inside.sum() > 100 and np.all(g_r[inside] < 0.0)
    # the ghost zone of the gravity FAB is the Gravity_Type fill of the valid zones: first-order extrapolation beyond outflow
    G = ref.grav_new.numpy()
    assert np.array_equal(G[:, 0, 1:-1, 1:-1], G[:, 1, 1:-1, 1:-1]) and np.array_equal(G[:, 1:-1, 1:-1, -1], G[:, 1:-1, 1:-1, -2])
    tol = np.maximum(1e-10, 100.0 * s)
    d = MR.field_deviation(ref.S_new().numpy(), free.S_new().numpy())
    assert d[MR.UMX] > 1e4 * tol[MR.UMX], (d, tol)
    assert np.all(s < 1e-8)
    st = ref.poisson_stats()
    print("cycles: first %d, last old-time %d, last new-time %d" % (st["first"]["cycles"], st["old"]["cycles"], st["new"]["cycles"]))
    assert st["new"]["cycles"] < st["first"]["cycles"] and st["old"]["cycles"] < st["first"]["cycles"]
    tolr = max(1e-10 * st["new"]["history"][0], 1e-10 * st["new"]["history"][1])
    assert st["new"]["norm"] <= tolr
    phi = ref.phi_grav().numpy()
    assert phi.shape == (1, 18, 18, 18) and np.all(phi < 0.0)
    # the potential at the centre of a uniform sphere is -3 G M / (2 R): the 16^3 solve is within 5 % of it
    M = 4.0 / 3.0 * np.pi * R.DUST_PROB["r_0"] ** 3 * R.DUST_PROB["rho_0"]
    assert abs(phi[0, 1:-1, 1:-1, 1:-1].min() / (-1.5 * 6.67428e-8 * M / R.DUST_PROB["r_0"]) - 1.0) < 0.05


def test_maxiter_one_raises(oracle):
    import castro_amd
    c = castro_amd.Castro(R.DUST_N, poisson=castro_amd.PoissonGravity(maxiter=1), **R.DUST_GEOM,
                          **_kw(oracle, params=oracle.default_params(**R.DUST_PARAMS)))
    c.center = R.DUST_CENTER
    c.initData("dust_collapse", **R.DUST_PROB)
    with pytest.raises(RuntimeError, match="last two residual norms"):
        c.step()


def test_plan_lifetime(oracle):
    """one plan after a step, none after close(), one again after the next step; the object stays with its driver"""
    import castro_amd
    c, _ = R.dust_collapse_run(R.PoissonOracleBackend(), oracle.default_params(**R.DUST_PARAMS), steps=1)
    R.assert_plan_lifetime(c)
    with pytest.raises(ValueError, match="one Castro"):
        castro_amd.Castro(R.DUST_N, poisson=c.poisson, **R.DUST_GEOM, **_kw(oracle))

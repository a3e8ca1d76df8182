"""GPU tests of castro_amd_integrated_quantities_mf (castro_amd/csrc/diag_kernels.hip) and of sum_integrated_quantities() of
the two drivers, for both numerics builds.  Reference and tolerance: tests/diag_ref.py (exactly rounded sums of the oracle's
per-zone terms; bound N 2^-52 A for the `exact` build, plus 1e-10 N vol max|field| for `contract`).

Observed deviation over the bound, worst of all quantities and cases of this file (printed by every comparison):
see DESIGN.md section 7."""
import numpy as np
import pytest
import torch

from tests import diag_ref
from tests.util import physical_state

pytestmark = pytest.mark.gpu

CENTER = (0.3, 0.55, 0.4)
N_CELL = (64, 64, 64)            # unit domain: dx = 1/64


@pytest.fixture(scope="module", params=["exact", "contract"])
def hydro(request):
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=request.param)
    yield h
    h.close()


def _geom():
    from castro_amd import _lib
    return _lib.make_geom(N_CELL)


def _box(seed, lo, ext, ng, nan_ghosts=True):
    """(valid state as numpy, FAB on the device with NaN ghost zones, box of the FAB, lo, hi)"""
    rng = np.random.default_rng(seed)
    hi = tuple(lo[d] + ext[d] - 1 for d in range(3))
    U = physical_state(rng, lo, hi, jump=False)
    assert U[0].min() > 0.0 and all(np.abs(U[c]).min() > 0.0 for c in (1, 2, 3))
    F = np.full((8, ext[2] + 2 * ng, ext[1] + 2 * ng, ext[0] + 2 * ng), np.nan if nan_ghosts else 0.0)
    F[:, ng:ng + ext[2], ng:ng + ext[1], ng:ng + ext[0]] = U
    fbox = (tuple(x - ng for x in lo), tuple(x + ng for x in hi))
    return U, torch.from_numpy(F).cuda(), fbox, lo, hi


def _call(h, specs, out=None, stream=None):
    """specs: [(fab tensor, fbox, lo, hi, mask tensor or None)] -> the 14 sums as numpy"""
    if out is None:
        out = torch.full((14,), float("nan"), dtype=torch.float64, device="cuda")
    boxes = h.make_diag_boxes([(lo, hi, (F, fbox), mask) for F, fbox, lo, hi, mask in specs])
    h.integrated_quantities_mf(boxes, _geom(), CENTER, out, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), boxes


def _check(h, got, ref, what):
    bound = diag_ref.bounds(ref, h.numerics)
    ratios = [abs(got[m] - ref["S"][m]) / bound[m] for m in range(14)]
    print("diag %s [%s]: worst deviation / bound = %.3g (%s), N = %d" % (what, h.numerics, max(ratios),
                                                                       diag_ref.NAMES[int(np.argmax(ratios))], ref["N"]))
    assert np.isfinite(got).all()
    for m in range(14):
        assert abs(got[m] - ref["S"][m]) <= bound[m], (diag_ref.NAMES[m], got[m], ref["S"][m], bound[m])
        assert ref["A"][m] > 0.0 and abs(ref["S"][m]) > 0.0            # no quantity is trivially zero


def _ref(oracle, boxes):
    return diag_ref.reference(oracle, boxes, oracle.make_geom(N_CELL), oracle.default_params(), CENTER)


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_one_box_with_awkward_extents_and_nan_ghost_zones(hydro, oracle):
    """lo = (3, 5, 2), 15 x 12 x 10 in a FAB with 4 ghost zones: an odd row length, rows that start on an odd zone, fewer zones
    than one workgroup takes; the ghost zones are NaN and must never be loaded"""
    U, F, fbox, lo, hi = _box(1, (3, 5, 2), (15, 12, 10), 4)
    got, boxes = _call(hydro, [(F, fbox, lo, hi, None)])
    assert hydro.diag_workgroups(boxes) == 1
    _check(hydro, got, _ref(oracle, [(U, lo, None)]), "one box 15x12x10")


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_many_rows_of_partial_sums(hydro, oracle):
    U, F, fbox, lo, hi = _box(2, (0, 0, 0), (64, 32, 32), 4)
    got, boxes = _call(hydro, [(F, fbox, lo, hi, None)])
    assert hydro.diag_workgroups(boxes) >= 8                      # 32: k_diag_final adds 32 rows
    _check(hydro, got, _ref(oracle, [(U, lo, None)]), "64x32x32")


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_box_table_of_unequal_boxes_is_deterministic(hydro, oracle):
    """four boxes in one call, FABs with 4, 0, 2 and 3 ghost zones (odd and even row strides, rows starting on either parity)"""
    made = [_box(10, (0, 0, 0), (16, 16, 16), 4), _box(11, (20, 1, 3), (15, 8, 8), 0),
            _box(12, (40, 8, 8), (32, 16, 8), 2), _box(13, (3, 30, 30), (8, 8, 24), 3)]
    specs = [(F, fbox, lo, hi, None) for _, F, fbox, lo, hi in made]
    got, boxes = _call(hydro, specs)
    assert hydro.diag_workgroups(boxes) == 6
    _check(hydro, got, _ref(oracle, [(U, lo, None) for U, _, _, lo, _ in made]), "four boxes")
    again, _ = _call(hydro, specs)
    assert got.tobytes() == again.tobytes()                       # (b) the same bits on every call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other, _ = _call(hydro, specs, stream=side)
    assert got.tobytes() == other.tobytes()                       # (c) and on another stream


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_masked_zones_are_skipped_not_multiplied(hydro, oracle):
    U, F, fbox, lo, hi = _box(1, (3, 5, 2), (15, 12, 10), 4)
    mask = np.ones((10, 12, 15), dtype=np.uint8)
    mask[3:7, 2:6, 9:15] = 0                                      # 6 x 4 x 4 zones up to the high x face of the box
    Fn = F.clone()
    hole = torch.from_numpy(mask == 0).cuda()
    Fn[:, 4:14, 4:16, 4:19][:, hole] = float("nan")
    Un = U.copy()
    Un[:, mask == 0] = np.nan
    got, _ = _call(hydro, [(Fn, fbox, lo, hi, torch.from_numpy(mask).cuda())])
    ref = _ref(oracle, [(Un, lo, mask)])
    assert ref["N"] == 15 * 12 * 10 - 96
    _check(hydro, got, ref, "masked 15x12x10")
    zero, _ = _call(hydro, [(Fn, fbox, lo, hi, torch.zeros((10, 12, 15), dtype=torch.uint8, device="cuda"))])
    assert zero.tobytes() == np.zeros(14).tobytes()               # +0.0, fourteen times
    ones, _ = _call(hydro, [(F, fbox, lo, hi, torch.ones((10, 12, 15), dtype=torch.uint8, device="cuda"))])
    none, _ = _call(hydro, [(F, fbox, lo, hi, None)])
    assert ones.tobytes() == none.tobytes()


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_no_boxes_writes_zeros_over_garbage(hydro):
    out = torch.full((14,), 1.234e300, dtype=torch.float64, device="cuda")
    out[3] = float("nan")
    got, _ = _call(hydro, [], out=out)
    assert got.tobytes() == np.zeros(14).tobytes()


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_uniform_state_on_a_power_of_two_grid_gives_the_closed_forms(hydro):
    """rho = 2, u = (0.5, 0, 0) on the whole 64^3 unit domain: every term and every partial sum is a dyadic rational"""
    n = 64
    F = torch.zeros((8, n, n, n), dtype=torch.float64, device="cuda")
    F[0], F[1], F[4], F[5], F[6], F[7] = 2.0, 1.0, 3.0, 2.75, 1.0, 2.0
    got, _ = _call(hydro, [(F, ((0, 0, 0), (n - 1,) * 3), (0, 0, 0), (n - 1,) * 3, None)])
    from castro_amd import _lib as L
    assert got[L.DIAG_MASS] == 2.0 and got[L.DIAG_XMOM] == 1.0 and got[L.DIAG_YMOM] == 0.0 and got[L.DIAG_ZMOM] == 0.0
    assert got[L.DIAG_RHO_K] == 0.25                              # 0.5 / rho * |rho u|^2 = 0.25 per unit volume
    assert got[L.DIAG_RHO_E] == 3.0 and got[L.DIAG_RHO_E_INT] == 2.75 and got[L.DIAG_SPECIES] == 2.0
    assert [got[L.DIAG_COM_X + d] / got[L.DIAG_MASS] for d in range(3)] == [0.5, 0.5, 0.5]
    # L = (loc - c) x (rho u) with rho u = (1, 0, 0): L_y = mean(z - cz), L_z = -mean(y - cy)
    assert got[L.DIAG_ANGMOM_X] == 0.0
    assert abs(got[L.DIAG_ANGMOM_Y] - (0.5 - CENTER[2])) <= n ** 3 * 2.0 ** -52 * 0.5
    assert abs(got[L.DIAG_ANGMOM_Z] + (0.5 - CENTER[1])) <= n ** 3 * 2.0 ** -52 * 0.5


# 7 ---------------------------------------------------------------------------------------------------------------------
def _sedov(numerics, **kw):
    import castro_amd
    c = castro_amd.Castro((32, 32, 32), numerics=numerics, **kw)
    c.initData("sedov", r_init=0.1, nsub=4)
    return c


@pytest.mark.parametrize("numerics", ["exact", "contract"])
def test_single_level_driver_sums_every_step_and_conserves(numerics, tmp_path):
    c = _sedov(numerics, sum_interval=1, diag_dir=str(tmp_path))
    for _ in range(4):
        c.step()
    H = c.diag_history
    assert [q["nstep"] for q in H] == [0, 1, 2, 3, 4] and H[0]["time"] == 0.0 and H[0]["dt"] == 0.0
    assert all(b["time"] > a["time"] for a, b in zip(H[:-1], H[1:])) and H[4]["time"] == c.time
    # no outflow: the blast has not reached the boundary -- the outermost layer still holds the ambient density
    rho = c.S_new()[0]
    for face in (rho[0], rho[-1], rho[:, 0], rho[:, -1], rho[:, :, 0], rho[:, :, -1]):
        assert bool((face == 1.0).all())
    N = 32 ** 3
    for a, b in zip(H[:-1], H[1:]):
        dm, de = abs(a["mass"] - b["mass"]), abs(a["rho_E"] - b["rho_E"])
        print("diag conservation [%s] step %d: dmass / bound = %.3g, dE / bound = %.3g"
              % (numerics, b["nstep"], dm / (N * 2.0 ** -52 * a["mass"]), de / (N * 2.0 ** -52 * a["rho_E"])))
        assert dm <= N * 2.0 ** -52 * a["mass"]
        assert de <= N * 2.0 ** -52 * a["rho_E"]
    direct = c.sum_integrated_quantities()
    assert all(direct[k] == H[4][k] for k in direct)
    from castro_amd import diag
    names, rows = diag.read_grid_diag(str(tmp_path / "grid_diag.out"))
    assert len(rows) == 5 and [r[1] for r in rows] == [q["mass"] for q in H]
    # batches capped at the next sum: the same physics as the default, bit for bit
    a, b = _sedov(numerics, sum_interval=2), _sedov(numerics)
    a.evolve(1.0, max_step=4)
    b.evolve(1.0, max_step=4)
    assert a.nstep == b.nstep == 4 and a.time == b.time and torch.equal(a.S_new(), b.S_new())
    assert [q["nstep"] for q in a.diag_history] == [0, 2, 4] and b.diag_history == []
    for x in (a, b, c):
        x.close()


# 8 ---------------------------------------------------------------------------------------------------------------------
def _composite_abs(amr, comp):
    """(sum of |S| vol, contributing zones) over the composite grid, the masks built here from the box lists"""
    from castro_amd import cluster as CL
    tot, N = 0.0, 0
    for l, lev in enumerate(amr.lev):
        v = lev.geom.dx[0] * lev.geom.dx[1] * lev.geom.dx[2]
        for b in lev.boxes:
            S = b.S_new()[comp].abs()
            keep = torch.ones_like(S, dtype=torch.bool)
            if l + 1 < len(amr.lev):
                o = b.lo
                for f in amr.lev[l + 1].boxes:
                    it = CL.intersect(f.pbox, b.bx)
                    if it:
                        (p, q) = it
                        keep[p[2] - o[2]:q[2] - o[2] + 1, p[1] - o[1]:q[1] - o[1] + 1, p[0] - o[0]:q[0] - o[0] + 1] = False
            tot += float(S[keep].sum().item()) * v
            N += int(keep.sum().item())
    return tot, N


def _amr_agrees(a, numerics, what):
    q = a.sum_integrated_quantities()
    for name, comp, got in (("mass", 0, q["mass"]), ("xmom", 1, q["mom"][0]), ("ymom", 2, q["mom"][1]), ("zmom", 3, q["mom"][2]),
                            ("rho_E", 4, q["rho_E"])):
        want = a.composite_sum(comp)
        A, N = _composite_abs(a, comp)
        bound = N * 2.0 ** -52 * A
        print("diag amr %s [%s] %s: |diff| / bound = %.3g, N = %d" % (what, numerics, name, abs(got - want) / bound, N))
        assert abs(got - want) <= bound, (name, got, want, bound)
    return q


@pytest.mark.parametrize("numerics", ["exact", "contract"])
def test_amr_driver_agrees_with_composite_sum_and_rebuilds_its_masks(numerics):
    import castro_amd
    a = castro_amd.CastroAmr((32, 32, 32), patch_crse=((6, 6, 6), (25, 25, 25)), sum_interval=1,
                             make_hydro=lambda: castro_amd.HipHydro(0, numerics=numerics))
    a.initData("sedov", r_init=0.1, nsub=4)
    a.step()
    a.step()
    assert len(a.lev) == 2 and [q["nstep"] for q in a.diag_history] == [0, 1, 2]
    q = _amr_agrees(a, numerics, "fixed patch")
    assert all(q[k] == a.diag_history[-1][k] for k in q)
    m = a._diag_level_masks(0)[a.lev[0].boxes[0].bx]
    assert int(m.sum().item()) == 32 ** 3 - 20 ** 3 and a._diag_level_masks(1) is None
    key = a._diag_mask_key(0)
    # a regrid that moves the patch: the tags follow the energy of the blast
    a.refine, a.max_level, a.blocking_factor = [("rho_E", "value_greater", 1.0)], 1, 4
    assert a.regrid() and len(a.lev) == 2 and a.pbox[1] != ((6, 6, 6), (25, 25, 25))
    assert a._diag_masks == {} and a._diag_mask_key(0) != key
    _amr_agrees(a, numerics, "after regrid")
    plo, phi = a.pbox[1]
    m2 = a._diag_level_masks(0)[a.lev[0].boxes[0].bx]
    assert int(m2.sum().item()) == 32 ** 3 - int(np.prod([phi[d] - plo[d] + 1 for d in range(3)]))

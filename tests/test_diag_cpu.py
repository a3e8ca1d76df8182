"""CPU tests of the integrated-quantity diagnostics (Castro::sum_integrated_quantities): the reference the GPU tests compare
against, the data-log writer, the trigger logic of the two drivers on the oracle-backed driver, allreduce_sum over gloo, and
the host arithmetic of the C ABI (box-table checks, workgroup count) -- none of it needs a GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import diag_ref
from tests.oracle_backend import OracleBackend
from tests.test_driver_cpu import _free_port
from tests.util import physical_state


class DiagOracleBackend(OracleBackend):
    """tests/oracle_backend.py plus the integrated quantities, summed with numpy (tests/diag_ref.py::numpy_sums)"""

    @staticmethod
    def make_diag_boxes(specs):
        return list(specs), len(specs)

    def integrated_quantities_mf(self, boxes, geom, center, out, stream=None):
        specs, n = boxes
        todo = []
        for lo, hi, (state, box), mask in specs[:n]:
            sl = self._slices(box, lo, hi)
            todo.append((state[sl].numpy(), lo, None if mask is None else mask.numpy()))
        out.copy_(torch.from_numpy(diag_ref.numpy_sums(todo, geom, center)))


# ---- the reference itself -------------------------------------------------------------------------------------------
def _hand_state():
    U = np.zeros((8, 4, 4, 4))
    rho = 1.0 + np.arange(4, dtype=np.float64)[None, None, :] + np.zeros((4, 4, 4))
    U[0], U[1], U[4], U[5], U[6], U[7] = rho, 2.0 * rho, 3.0 * rho, 0.5 * rho, 1.0, 0.25 * rho
    return U


def test_diag_ref_against_hand_computed_sums_on_a_4_cubed_state(oracle):
    """rho = 1 + i, rho u = (2 rho, 0, 0) on the unit cube cut into 4^3 zones (vol = 1/64), centre (0.5, 0.25, 0.5): every term
    and every partial sum is a dyadic rational, so the closed forms hold with ==.
      mass = 16/64 (1+2+3+4) = 2.5; xmom = 5; rho_K = sum 0.5/rho (2 rho)^2 vol = sum 2 rho vol = 5; rho_E = 7.5; rho_e = 1.25
      L_z = sum ((x - cx) my - (y - cy) mx) vol = -mean(y - 0.25) * xmom = -0.25 * 5;  L_x = L_y = 0 (z symmetric about cz)
      sum rho x vol = 0.25 (1 * .125 + 2 * .375 + 3 * .625 + 4 * .875) = 1.5625;  sum rho y vol = sum rho z vol = 0.5 * 2.5"""
    U, geom, P, c = _hand_state(), oracle.make_geom((4, 4, 4)), oracle.default_params(), (0.5, 0.25, 0.5)
    want = [2.5, 5.0, 0.0, 0.0, 0.0, 0.0, -1.25, 1.25, 5.0, 7.5, 1.5625, 1.25, 1.25, 0.625]
    ref = diag_ref.reference(oracle, [(U, (0, 0, 0), None)], geom, P, c)
    assert ref["S"] == want and ref["N"] == 64
    assert ref["A"][0] == 2.5 and ref["A"][6] == 5.0 * (0.125 + 0.125 + 0.375 + 0.625) / 4     # sum |y - cy| / 4 = 0.3125
    assert list(diag_ref.numpy_sums([(U, (0, 0, 0), None)], geom, c)) == want
    # a mask dropping the plane i = 3 (and a NaN under it): mass = 16/64 (1+2+3)
    mask = np.ones((4, 4, 4), dtype=np.uint8)
    mask[:, :, 3] = 0
    Un = U.copy()
    Un[:, :, :, 3] = np.nan
    ref = diag_ref.reference(oracle, [(Un, (0, 0, 0), mask)], geom, P, c)
    assert ref["N"] == 48 and ref["S"][0] == 1.5 and ref["S"][1] == 3.0 and ref["S"][10] == 0.25 * (0.125 + 0.75 + 1.875)
    assert all(np.isfinite(ref["S"])) and all(np.isfinite(ref["A"]))
    # two boxes are the union: the same cube as two slabs in z, the second one with its own lo
    ref2 = diag_ref.reference(oracle, [(U[:, :2], (0, 0, 0), None), (U[:, 2:], (0, 0, 2), None)], geom, P, c)
    assert ref2["S"] == want
    # the tolerances: exact N 2^-52 A; contract adds 1e-10 N vol max|field|
    be, bc = diag_ref.bounds(ref2, "exact"), diag_ref.bounds(ref2, "contract")
    assert be[0] == 64 * 2.0 ** -52 * 2.5 and bc[0] == be[0] + 1e-10 * 64 * (1.0 / 64) * 4.0
    assert bc[6] > be[6] and ref2["fmax"][6] >= 8.0 * 0.375            # |loc - c| |rho u| of a far zone, not the cancelled product


# ---- the data logs --------------------------------------------------------------------------------------------------
def test_grid_diag_log_round_trips_in_the_reference_layout(tmp_path):
    from castro_amd import diag
    log = diag.DiagLog(sum_interval=1, diag_dir=str(tmp_path))
    rng = np.random.default_rng(5)
    qs = []
    for n in range(3):
        v = list(rng.standard_normal(14) * 10.0 ** rng.integers(-30, 30, 14))
        v[0] = abs(v[0]) + 1.0
        q = diag.quantities(0.0 if n == 0 else 1.0e-3 * n / 3.0, v)
        log.begin_steps(1)
        qs.append(log.record(q, n, 0.0 if n == 0 else 1.0e-3 / 3.0))
    names, rows = diag.read_grid_diag(str(tmp_path / "grid_diag.out"))
    # the reference's order: rho_K in front of rho_e
    assert names == ["time", "mass", "xmom", "ymom", "zmom", "ang mom x", "ang mom y", "ang mom z", "rho_K", "rho_e", "rho_E"]
    assert len(rows) == 3
    for q, row in zip(qs, rows):
        want = [q["time"], q["mass"]] + q["mom"] + q["ang_mom"] + [q["rho_K"], q["rho_e"], q["rho_E"]]
        assert row == want                                 # 17 significant digits: the doubles come back exactly
    lines = open(tmp_path / "grid_diag.out").read().splitlines()
    assert len(lines) == 4 and all(len(ln) == 11 * 25 for ln in lines)           # width 25 per column, header included
    assert sum(1 for ln in lines if "mass" in ln) == 1
    assert "%25.16e" % qs[1]["mass"] == lines[2][25:50]                         # precision 16, scientific
    sp = open(tmp_path / "species_diag.out").read().splitlines()
    assert len(sp) == 5 and sp[0].startswith("#   COLUMN 1") and "Mass X" in sp[1] and float(sp[3].split()[2]) == qs[1]["species_mass"][0]
    am = open(tmp_path / "amr_diag.out").read().splitlines()
    assert len(am) == 5 and "COARSE TIMESTEP WALLTIME" in am[1]
    step, t, dt, finest, wall = am[3].split()
    assert (int(step), int(finest)) == (1, 0) and abs(float(dt) - 1.0e-3 / 3.0) < 1e-16 and float(wall) >= 0.0
    assert float(am[2].split()[2]) == 0.0 and float(am[2].split()[4]) == 0.0    # time 0: dt and the wall time are reported as 0
    # a new time-0 entry starts the files again: one header row, always
    log.reset()
    log.record(diag.quantities(0.0, [1.0] * 14), 0, 0.0)
    assert len(open(tmp_path / "grid_diag.out").read().splitlines()) == 2
    assert diag.quantities(0.0, [2.0] + [1.0] * 13)["com"] == [0.5] * 3 and diag.quantities(0.0, [2.0] + [1.0] * 13)["com_vel"] == [0.5] * 3
    from castro_amd import _lib
    assert diag.quantities(0.0, [1.0] * 14)["species_mass"] == [1.0 / _lib.M_SOLAR] and _lib.M_SOLAR == 1.9884e33


# ---- the trigger logic on the oracle-backed driver --------------------------------------------------------------------
def _castro(oracle, n=(16, 16, 16), **kw):
    import castro_amd
    c = castro_amd.Castro(n, params=oracle.default_params(), hydro=DiagOracleBackend(), **kw)
    c.initData("sedov", r_init=0.1, nsub=4)
    return c


def test_sum_interval_triggers_after_init_and_every_interval_steps(oracle, tmp_path):
    c = _castro(oracle, sum_interval=2, diag_dir=str(tmp_path))
    assert [(q["nstep"], q["time"], q["dt"]) for q in c.diag_history] == [(0, 0.0, 0.0)]
    for _ in range(5):
        c.step()
    assert [q["nstep"] for q in c.diag_history] == [0, 2, 4]
    assert c.diag_history[1]["time"] > 0.0 and c.diag_history[2]["time"] > c.diag_history[1]["time"] and c.diag_history[2]["dt"] > 0.0
    # conservation: the blast is far from the (outflow) boundary, so mass and total energy stay within the summation bound
    N = 16 ** 3
    for a, b in zip(c.diag_history[:-1], c.diag_history[1:]):
        assert abs(a["mass"] - b["mass"]) <= N * 2.0 ** -52 * a["mass"]
        assert abs(a["rho_E"] - b["rho_E"]) <= N * 2.0 ** -52 * a["rho_E"]
    # the entry of the last due step is what a direct call gives for that state
    c2 = _castro(oracle, sum_interval=2)
    for _ in range(4):
        c2.step()
    direct = c2.sum_integrated_quantities()
    assert all(direct[k] == c.diag_history[2][k] for k in direct)
    from castro_amd import diag
    names, rows = diag.read_grid_diag(str(tmp_path / "grid_diag.out"))
    assert [r[0] for r in rows] == [q["time"] for q in c.diag_history] and [r[1] for r in rows] == [q["mass"] for q in c.diag_history]
    # a new initData starts the history again
    c.initData("sedov", r_init=0.1, nsub=4)
    assert [q["nstep"] for q in c.diag_history] == [0]
    # the default: nothing is summed, nothing is written
    d = _castro(oracle)
    d.step()
    assert d.sum_interval == -1 and d.diag_history == []


def test_evolve_caps_its_batches_at_the_next_sum_and_changes_no_physics(oracle):
    from castro_amd.diag import DiagLog
    log = DiagLog(sum_interval=4)
    assert [log.cap(10, n) for n in (0, 1, 3, 4, 7)] == [4, 3, 1, 4, 1] and log.cap(2, 4) == 2
    assert DiagLog().cap(10, 3) == 10 and not DiagLog().due(4)                  # sum_interval = -1: batches are not touched
    assert log.due(8) and not log.due(9)
    log.last_nstep = 8
    assert not log.due(8)                                                       # a step is summed once
    a, b = _castro(oracle, sum_interval=2), _castro(oracle)
    a.evolve(1.0, max_step=4)
    b.evolve(1.0, max_step=4)
    assert a.nstep == b.nstep == 4 and a.time == b.time
    assert torch.equal(a.S_new(), b.S_new())
    assert [q["nstep"] for q in a.diag_history] == [0, 2, 4] and b.diag_history == []


def test_amr_driver_masks_the_covered_zones_and_rebuilds_after_a_regrid(oracle):
    import castro_amd
    from castro_amd import cluster as CL
    a = castro_amd.CastroAmr((16, 16, 16), patch_crse=((2, 2, 2), (11, 11, 11)), params=oracle.default_params(),
                             make_hydro=DiagOracleBackend, sum_interval=1)
    a.initData("sedov", r_init=0.1, nsub=4)
    a.step()
    a.step()
    assert [q["nstep"] for q in a.diag_history] == [0, 1, 2] and a.diag_history[-1]["finest_level"] == 1
    q = a.sum_integrated_quantities()
    assert q == {k: a.diag_history[-1][k] for k in q}
    N = 16 ** 3 - 10 ** 3 + 20 ** 3
    for comp, got in ((0, q["mass"]), (4, q["rho_E"])):
        want = a.composite_sum(comp)
        assert abs(got - want) <= N * 2.0 ** -52 * abs(want)
    m = a._diag_level_masks(0)[a.lev[0].boxes[0].bx].numpy()
    assert m.dtype == np.uint8 and m.sum() == 16 ** 3 - 10 ** 3 and not m[2:12, 2:12, 2:12].any()
    assert a._diag_level_masks(1) is None
    key = a._diag_mask_key(0)
    assert a._diag_level_masks(0)[a.lev[0].boxes[0].bx] is a._diag_level_masks(0)[a.lev[0].boxes[0].bx]      # cached between regrids
    # a regrid that moves the patch: tags where the energy of the blast is, a smaller box than the fixed one
    a.refine, a.max_level, a.blocking_factor = [("rho_E", "value_greater", 1.0)], 1, 4
    assert a.regrid() and a.pbox[1] == ((4, 4, 4), (11, 11, 11))
    assert a._diag_masks == {} and a._diag_mask_key(0) != key
    q2 = a.sum_integrated_quantities()
    plo, phi = a.pbox[1]
    m2 = a._diag_level_masks(0)[a.lev[0].boxes[0].bx].numpy()
    assert m2.sum() == 16 ** 3 - int(np.prod([phi[d] - plo[d] + 1 for d in range(3)]))
    for comp, got in ((0, q2["mass"]), (4, q2["rho_E"])):
        want = a.composite_sum(comp)
        assert abs(got - want) <= 2 * 16 ** 3 * 2.0 ** -52 * abs(want)
    assert CL.intersect((plo, phi), ((0, 0, 0), (15, 15, 15))) == (plo, phi)


# ---- allreduce_sum ----------------------------------------------------------------------------------------------------
def test_single_comm_allreduce_sum_is_the_identity():
    import castro_amd
    t = torch.arange(14, dtype=torch.float64)
    assert castro_amd.SingleComm().allreduce_sum(t) is t and torch.equal(t, torch.arange(14, dtype=torch.float64))


def _sum_worker(rank, world, port, n, out_path):
    import torch.distributed as dist
    import castro_amd
    from oracle import oracle_lib as O
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = castro_amd.Castro(n, params=O.default_params(), hydro=DiagOracleBackend(), comm=castro_amd.DistComm())
        c.center = (0.3, 0.55, 0.4)
        c.set_state(physical_state(np.random.default_rng(11), (0, 0, 0), tuple(x - 1 for x in n), jump=False))
        q = c.sum_integrated_quantities()
        t = torch.full((3,), float(rank + 1), dtype=torch.float64)
        c.comm.allreduce_sum(t)
        if rank == 0:
            with open(out_path, "w") as f:
                json.dump(dict(q=q, t=t.tolist(), box=[c.lo, c.hi]), f)
    finally:
        dist.destroy_process_group()


def test_two_half_domain_ranks_give_the_sums_of_the_undivided_domain_gloo(tmp_path, oracle):
    import castro_amd
    n = (8, 8, 16)
    out = str(tmp_path / "sum.json")
    mp.spawn(_sum_worker, args=(2, _free_port(), n, out), nprocs=2, join=True)
    got = json.load(open(out))
    assert got["t"] == [3.0, 3.0, 3.0] and got["box"] == [[0, 0, 0], [7, 7, 7]]           # two halves along z
    # the undivided domain: the same initial data through the same post-init clean_state on one rank
    c = castro_amd.Castro(n, params=oracle.default_params(), hydro=DiagOracleBackend())
    c.set_state(physical_state(np.random.default_rng(11), (0, 0, 0), tuple(x - 1 for x in n), jump=False))
    center = (0.3, 0.55, 0.4)
    ref = diag_ref.reference(oracle, [(c.S_new().numpy().copy(), (0, 0, 0), None)], c.geom, c.params, center)
    bound = diag_ref.bounds(ref, "exact")
    q = got["q"]
    vec = [q["mass"]] + q["mom"] + q["ang_mom"] + [q["rho_e"], q["rho_K"], q["rho_E"]]
    for m, v in enumerate(vec):
        assert abs(v - ref["S"][m]) <= bound[m], (diag_ref.NAMES[m], v, ref["S"][m], bound[m])
    for d in range(3):
        assert abs(q["com"][d] * q["mass"] - ref["S"][10 + d]) <= bound[10 + d] + 2.0 ** -52 * abs(ref["S"][10 + d])
    assert min(abs(v) for v in vec) > 0.0                                   # no quantity is trivially zero


# ---- the C ABI without a device: box-table checks and launch geometry ------------------------------------------------------
def _diag_boxes(specs):
    """[(lo, extents, ghosts)] -> castro_amd_diag_box array over host memory (only the alignment of the pointer is looked at)"""
    from castro_amd import _lib
    arr = (_lib.DiagBox * len(specs))()
    keep = []
    for db, (lo, ext, ng) in zip(arr, specs):
        flo = tuple(x - ng for x in lo)
        fhi = tuple(lo[d] + ext[d] - 1 + ng for d in range(3))
        buf = np.zeros(8, dtype=np.float64)
        keep.append(buf)
        for d in range(3):
            db.lo[d], db.hi[d] = lo[d], lo[d] + ext[d] - 1
        db.state = _lib.fab_desc(buf.ctypes.data, flo, fhi, 8)
    return arr, keep


def test_diag_box_binding_and_launch_geometry_without_a_device():
    import __graft_entry__ as g
    from castro_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    assert C.sizeof(_lib.DiagBox) == 2 * 12 + 40 + 8 and _lib.DIAG_N == 14      # castro_amd_diag_box (LP64)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "castro_hydro_amd.h")).read()
    for name in ("MASS", "XMOM", "YMOM", "ZMOM", "ANGMOM_X", "ANGMOM_Y", "ANGMOM_Z", "RHO_E_INT", "RHO_K", "RHO_E", "COM_X", "COM_Y",
                 "COM_Z", "SPECIES"):
        assert "#define CASTRO_AMD_DIAG_%s %d\n" % (name, getattr(_lib, "DIAG_" + name)) in hdr
    assert "#define CASTRO_AMD_DIAG_N 14" in hdr
    for mode in _lib.NUMERICS_MODES:
        lib = _lib.load(mode)
        arr, keep = _diag_boxes([((0, 0, 0), (64, 32, 32), 4)])
        # 32 pairs a row x 1024 rows, 256 threads x 4 pairs a workgroup
        assert lib.castro_amd_diag_workgroups(1, arr) == 32
        arr, keep = _diag_boxes([((3, 5, 2), (15, 12, 10), 4)])
        assert lib.castro_amd_diag_workgroups(1, arr) == 1
        arr, keep = _diag_boxes([((0, 0, 0), (16, 16, 16), 4), ((20, 1, 3), (15, 8, 8), 0), ((40, 8, 8), (32, 16, 8), 2),
                                 ((3, 30, 30), (8, 8, 24), 3)])
        assert lib.castro_amd_diag_workgroups(4, arr) == 2 + 1 + 2 + 1
        # the grid is capped: a thread takes more pairs instead (256^3: 128 pairs a row -> 2048 workgroups of 16 pairs a thread)
        arr, keep = _diag_boxes([((0, 0, 0), (256, 256, 256), 4)])
        assert lib.castro_amd_diag_workgroups(1, arr) == 2048
        assert lib.castro_amd_diag_workgroups(0, None) == 0
        # argument errors as in the neighbouring calls
        arr, keep = _diag_boxes([((0, 0, 0), (8, 8, 8), 0)])
        arr[0].state.ncomp = 7
        assert lib.castro_amd_diag_workgroups(1, arr) == _lib.ERR_ARG
        arr[0].state.ncomp = 8
        arr[0].hi[0] = 8                                   # valid box outside the FAB
        assert lib.castro_amd_diag_workgroups(1, arr) == _lib.ERR_ARG
        assert lib.castro_amd_diag_workgroups(-1, arr) == _lib.ERR_ARG and lib.castro_amd_diag_workgroups(1, None) == _lib.ERR_ARG
        out = (C.c_double * 14)()
        ctr = (C.c_double * 3)(0.5, 0.5, 0.5)
        geom = _lib.make_geom((8, 8, 8))
        assert lib.castro_amd_integrated_quantities_mf(None, 0, None, C.byref(geom), C.byref(ctr), out, None) == _lib.ERR_ARG

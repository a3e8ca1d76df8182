"""The boundary overrides of the state fill (hydrostatic Inflow faces, the ambient state beyond Outflow faces) without a GPU:
the numpy restatement (tests/ext_bc_ref.py) against the reference's own ambient_fill / hse_fill
(tests/golden/stub_probe/bc_vectors.npz, tests/ext_bc_cases.py), the Python interface, and the drivers on the oracle backend with
the restatement as their ext_bc_fill (tests/ext_bc_backend.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import ext_bc_cases as X
from tests import ext_bc_ref as R
from tests.ext_bc_backend import ExtBcOracleBackend
from tests.test_driver_cpu import _free_port, _hse_atmosphere

GAMMA = 1.4
# the atmosphere of the issue: slip walls in x and y, symmetry at +z, z low Inflow
ATMOS = dict(lo_bc=(4, 4, 1), hi_bc=(4, 4, 3), prob_hi=(0.125, 0.125, 1.0), do_grav=True, const_grav=-1.0)


def test_the_restatement_reproduces_the_reference_bit_for_bit():
    assert X.ncases() >= 25
    silent_cases = 0
    for c in range(X.ncases()):
        box, geom, params, ext, U_in, U_out, silent = X.case(c)
        U = U_in.copy()
        bad = R.ext_bc_fill(U, box, geom, params, ext)
        assert X.bits_equal(U, U_out), "bc%d" % c
        assert (bad > 0) == silent, "bc%d" % c
        silent_cases += silent
    assert silent_cases == 1


def test_the_cases_reach_what_they_are_there_for():
    V = X.vectors()
    # a FAB that does not reach the boundary: output == input
    assert X.bits_equal(V["out:bc14.U"], V["in:bc14.U"])
    # the scale height below dx needs more than two Newton iterations under the 10 % clamp: a density ratio above 1.1^2
    box, geom, _, _, _, U_out, _ = X.case(12)
    k0 = geom.domlo[2] - box[0][2]
    assert (U_out[0, k0 - 1] / U_out[0, k0]).min() > 1.1 ** 2
    # ambient_outflow_vel: in-domain normal momenta of both signs on a low and on a high face
    box, geom, _, ext, U_in, U_out, _ = X.case(21)
    i0, i1 = geom.domlo[0] - box[0][0], geom.domhi[0] - box[0][0]
    inner = (slice(geom.domlo[2] - box[0][2], geom.domhi[2] - box[0][2] + 1), slice(geom.domlo[1] - box[0][1], geom.domhi[1] - box[0][1] + 1))
    for edge, ghost, keep in ((i0, i0 - 1, np.minimum), (i1, i1 + 1, np.maximum)):
        m = U_in[(1,) + inner + (edge,)]
        assert (m > 0).any() and (m < 0).any()
        assert np.array_equal(U_out[(1,) + inner + (ghost,)], keep(0.0, m))
    # the `else if` chain: beyond an x wall and an ambient y face the x branch is taken -- the y momentum is zero there
    box, geom, _, _, U_in, U_out, _ = X.case(22)
    j = geom.domlo[1] - box[0][1] - 1
    k = geom.domlo[2] - box[0][2]
    assert U_out[2, k, j, 0] == 0.0 and U_out[2, k, j, geom.domlo[0] - box[0][0]] != 0.0
    # z low stores the temperature of every zone of the walk in the first ghost zone only (hse_fill.cpp:963); the last zone of a
    # walk of four extrapolates from two zones that still hold the generic fill, so the ghost zones end with the temperatures
    # they came with, although the densities were integrated with extrapolated ones.  An x face stores it zone by zone
    _, _, _, _, U_in, U_out, _ = X.case(8)
    assert X.bits_equal(U_out[6], U_in[6]) and not np.array_equal(U_out[0], X.case(4)[5][0])
    _, _, _, _, U_in, U_out, _ = X.case(11)
    assert not np.array_equal(U_out[6], U_in[6])


def test_make_ext_bc_defaults_and_the_ambient_state():
    from castro_amd import _lib as L
    assert C.sizeof(L.ExtBc) == 6 * 4 + 6 * 4 + 8 + 8 * 8          # castro_amd_ext_bc
    assert "castro_amd_ext_bc_fill_fab" in L.EXPORTED_SYMBOLS
    E = L.make_ext_bc()
    assert list(E.lo_type) == [-1] * 3 and list(E.hi_type) == [-1] * 3
    assert (E.hse_zero_vels, E.hse_interp_temp, E.hse_reflect_vels, E.fill_ambient_bc, E.ambient_fill_dir, E.ambient_outflow_vel) \
        == (0, 0, 0, 0, -1, 0)
    assert (E.ambient_density, E.ambient_temp, E.ambient_energy) == (-1.e200,) * 3
    E = L.make_ext_bc(xl="hse", xr=1, yl="none", zl=-1)
    assert list(E.lo_type) == [1, -1, -1] and list(E.hi_type) == [1, -1, -1]
    # Castro_setup.cpp:339-350
    P = L.default_params(small_dens=1.e-6, small_temp=1.e-3)
    assert L.ambient_state(P) == (P.small_dens, 0.0, 0.0, 0.0, P.small_dens * P.small_ener, P.small_dens * P.small_ener,
                                  P.small_temp, P.small_dens)
    ener = 4.0 * P.small_ener                      # a parameter counts where it is above the floor
    amb = L.ambient_state(P, ambient_density=0.25, ambient_temp=-5.0, ambient_energy=ener)
    assert amb == (0.25, 0.0, 0.0, 0.0, 0.25 * ener, 0.25 * ener, P.small_temp, 0.25)
    assert L.ambient_state(P, ambient_density=0.25, ambient_energy=0.5 * P.small_ener)[5] == 0.25 * P.small_ener
    F = L.complete_ext_bc(L.make_ext_bc(zl="hse", ambient_density=0.25, ambient_energy=ener), P, -2.5)
    assert F.const_grav == -2.5 and tuple(F.ambient_state) == L.ambient_state(P, 0.25, -1.e200, ener) and F.lo_type[2] == 1


def test_what_the_device_entry_refuses_raises_value_error(oracle):
    import castro_amd
    from castro_amd import _lib as L
    with pytest.raises(ValueError, match=r"\+Z"):
        L.make_ext_bc(zr="hse")
    with pytest.raises(ValueError, match="corner"):
        L.make_ext_bc(xl="hse", zl="hse")
    L.make_ext_bc(xl="hse", xr="hse")                       # opposite faces are fine
    for bad in ("HSE", 0, 2, True, None):
        with pytest.raises(ValueError):
            L.make_ext_bc(zl=bad)
    with pytest.raises(ValueError):
        L.make_ext_bc(ambient_fill_dir=3)
    ext = L.make_ext_bc(zl="hse")
    g = L.make_geom((4, 4, 8), lo_bc=(1, 2, 1), hi_bc=(2, 2, 2))
    with pytest.raises(ValueError, match="corner"):
        L.check_ext_bc(ext, g)
    g = L.make_geom((4, 4, 8), lo_bc=(2, 2, 1), hi_bc=(2, 2, 2))
    g.coord = 1
    with pytest.raises(ValueError, match="Cartesian"):
        L.check_ext_bc(ext, g)
    with pytest.raises(ValueError, match="two zones"):
        L.check_ext_bc(L.make_ext_bc(zl="hse", hse_interp_temp=1), L.make_geom((4, 4, 1), lo_bc=(2, 2, 1)))
    kw = dict(params=oracle.default_params(), hydro=ExtBcOracleBackend())
    with pytest.raises(ValueError, match="corner"):
        castro_amd.Castro((4, 4, 8), lo_bc=(1, 4, 1), hi_bc=(4, 4, 3), ext_bc=ext, **kw)
    with pytest.raises(ValueError, match="constant gravity"):
        castro_amd.Castro((8, 8, 8), lo_bc=(2, 2, 1), hi_bc=(2, 2, 2), ext_bc=ext, do_grav=True, gravity_type="monopole", **kw)
    # the restatement refuses what the entry refuses
    box, geom, params, e, U_in, _, _ = X.case(4)
    g = L.Geom.from_buffer_copy(geom)
    g.lo_bc[1] = 1
    with pytest.raises(ValueError):
        R.ext_bc_fill(U_in.copy(), box, g, params, e)


def _atmosphere_run(oracle, n, ext, steps, at=(), **kw):
    """the driver on the CPU; returns it and {step: (largest |w| / c in the lowest 8 layers, |relative mass change|)}"""
    import castro_amd
    c = castro_amd.Castro(n, params=oracle.default_params(**kw), hydro=ExtBcOracleBackend(), ext_bc=ext, **ATMOS)
    c.set_state(_hse_atmosphere(n))
    m0, out = c.S_new().numpy()[0].sum(), {}
    for s in range(1, steps + 1):
        c.step(1.0)
        if s in at:
            S = c.S_new().numpy()
            cs = np.sqrt(GAMMA * (GAMMA - 1.0) * S[5] / S[0])
            out[s] = (np.abs(S[3] / S[0] / cs)[:8].max(), abs(S[0].sum() / m0 - 1.0))
    return c, out


@pytest.fixture(scope="module")
def atmosphere(oracle):
    """the (4, 4, 32) atmosphere with an open lower boundary, PPM, 40 steps: extrapolated (today) and hydrostatic"""
    from castro_amd import _lib as L
    plain = _atmosphere_run(oracle, (4, 4, 32), None, 40, at=(12, 40))
    hse = _atmosphere_run(oracle, (4, 4, 32), L.make_ext_bc(zl="hse"), 40, at=(12, 40))
    return plain, hse


def test_the_atmosphere_stays_quiet_on_a_hydrostatic_lower_boundary(atmosphere):
    (cp, plain), (ch, hse) = atmosphere
    print("12 steps: |w|/c %.3g extrapolated, %.3g hydrostatic; 40 steps: mass change %.3g, %.3g"
          % (plain[12][0], hse[12][0], plain[40][1], hse[40][1]))
    assert cp.hydro.ext_fills == 0 and ch.hydro.ext_fills > 0
    assert hse[12][0] * 100.0 <= plain[12][0]
    assert hse[40][1] < 0.1 * plain[40][1]
    assert not ch.bc_in_hydro and not ch._light_overlap()


def test_an_unconverged_column_raises_where_the_step_reads_its_reduction(oracle):
    import castro_amd
    from castro_amd import _lib as L
    n = (4, 4, 32)
    c = castro_amd.Castro(n, params=oracle.default_params(), hydro=ExtBcOracleBackend(),
                          ext_bc=L.make_ext_bc(zl="hse", hse_interp_temp=1), **ATMOS)
    S = _hse_atmosphere(n)
    S[5, 0], S[5, 1] = 0.01 * S[5, 0], 100.0 * S[5, 1]          # a temperature that the extrapolation takes below zero
    S[4] = S[5]
    c.set_state(S)
    with pytest.raises(RuntimeError, match="z-low.*failed to converge"):
        c.step(1.0)


def _rank_worker(rank, world, port, n, grid, nsteps, out_path):
    import torch.distributed as dist
    import castro_amd
    from castro_amd import _lib as L
    from oracle import oracle_lib as O
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = castro_amd.Castro(n, params=O.default_params(), hydro=ExtBcOracleBackend(), comm=castro_amd.DistComm(), grid=grid,
                              ext_bc=L.make_ext_bc(zl="hse"), **ATMOS)
        c.set_state(_hse_atmosphere(n))
        for _ in range(nsteps):
            c.step(1.0)
        mine = c.S_new().contiguous()
        parts = [torch.zeros_like(mine) for _ in range(world)] if rank == 0 else None
        dist.gather(mine, parts, dst=0)
        boxes = c.comm.gather_objects((c.lo, c.hi))
        if rank == 0:
            full = np.zeros((8, n[2], n[1], n[0]))
            for p, (lo, hi) in zip(parts, boxes):
                full[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = p.numpy()
            np.save(out_path, full)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("grid", [(1, 1, 2), (2, 1, 1)])
def test_two_ranks_give_the_single_rank_state_gloo(tmp_path, oracle, grid):
    """split along z only the lower rank touches the hydrostatic face; split along x both do, and their ghost columns beyond
    the cut start from exchanged zones"""
    from castro_amd import _lib as L
    n, nsteps = (16, 4, 32), 4
    out = str(tmp_path / "ranks.npy")
    mp.spawn(_rank_worker, args=(2, _free_port(), n, grid, nsteps, out), nprocs=2, join=True)
    c, _ = _atmosphere_run(oracle, n, L.make_ext_bc(zl="hse"), nsteps)
    assert np.array_equal(np.load(out), c.S_new().numpy())


def _amr_atmosphere(oracle, ext, backend=ExtBcOracleBackend, params=None, n=(8, 8, 16)):
    """one refined patch sitting on the z-low boundary of an isothermal atmosphere (tools/amr_hse_validation.py)"""
    import castro_amd
    kw = dict(prob_hi=(0.5, 0.5, 1.0), lo_bc=(0, 0, 1), hi_bc=(0, 0, 3), do_grav=True, const_grav=-1.0,
              params=params if params is not None else oracle.default_params())
    a = castro_amd.CastroAmr(n, patches=[((2, 2, 0), (5, 5, 3))], make_hydro=backend, ext_bc=ext, **kw)
    H = 0.25
    for lev in a.levels:
        for b in lev.boxes:
            S = b.S_new()
            dz = 1.0 / ((2 ** lev.l) * n[2])
            z = (torch.arange(b.lo[2], b.hi[2] + 1, dtype=torch.float64) + 0.5) * dz
            rho = (torch.exp(-(z - 0.5 * dz) / H) - torch.exp(-(z + 0.5 * dz) / H)) * H / dz
            # made on the host whatever the backend (a device evaluates exp and a division by a scalar differently): the same
            # bits for the device run and its CPU twin
            host = torch.zeros(tuple(S.shape), dtype=torch.float64)
            host[0] = rho[:, None, None]
            host[7] = host[0]
            host[5] = host[0] * H / (GAMMA - 1.0)
            host[4] = host[5]
            S.copy_(host)
            b.clean_state(b.S_new_b, 1)
    return a


def amr_mach(a):
    out = 0.0
    for lev in a.levels:
        for b in lev.boxes:
            S = b.S_new()
            cs = torch.sqrt(GAMMA * (GAMMA - 1.0) * S[5] / S[0])
            out = max(out, (S[3] / S[0] / cs).abs().max().item())
    return out


def test_amr_patch_on_the_hydrostatic_boundary(oracle):
    from castro_amd import _lib as L
    a = _amr_atmosphere(oracle, L.make_ext_bc(zl="hse"))
    plain = _amr_atmosphere(oracle, None)
    fine = a.levels[1]
    b = fine.boxes[0]
    assert b.lo[2] == 0 and b.ext_bc is not None and b.ext_bc.const_grav == -1.0
    fine.alpha = 1.0                            # the coarse data under the fine ghost zones at the new time (the old one is empty)
    fine.fill("S_new_b")
    got = b.S_new_b.numpy().copy()
    want = got.copy()
    a.levels[1].hydro.bc_fill(torch.from_numpy(want), b.gbox, b.geom)           # the generic fill, then the restatement
    assert R.ext_bc_fill(want, b.gbox, b.geom, b.params, b.ext_bc) == 0
    below = got[:, :4]
    assert X.bits_equal(got, want)
    assert (np.diff(below[0], axis=0) < 0).all(), "the density grows downwards below the domain"
    plain.levels[1].alpha = 1.0
    plain.levels[1].fill("S_new_b")
    assert not np.array_equal(plain.levels[1].boxes[0].S_new_b.numpy()[:, :4], below)
    for _ in range(4):
        d = a.step(1.0)
        plain.step(1.0)
    assert d > 0.0
    print("largest |w|/c after 4 coarse steps: %.3g hydrostatic, %.3g extrapolated" % (amr_mach(a), amr_mach(plain)))
    assert amr_mach(a) < amr_mach(plain)


def test_amrex_adapter_ext_bc_fill_compiles_against_the_api_mock():
    """castro_amd::ext_bc_fill of include/castro_hydro_amd_amrex.H against the AMReX API mock (tests/mock_amrex/, as
    tests/test_capi_symbols.py does for the other entry points): syntax, types and overload resolution, against the C ABI header"""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-command-line-argument",
                        "-x", "hip", "--offload-arch=gfx950", "-I" + os.path.join(root, "tests", "mock_amrex"),
                        "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "mock_amrex", "adapter_ext_bc_tu.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_the_ambient_parameters_of_an_ext_bc_however_it_was_made(oracle):
    """castro.ambient_density / _temp / _energy ride beside the C struct: copy() and complete_ext_bc keep them, a struct built
    directly or copied as bytes has the reference's defaults (not set: the small_* quantities)"""
    from castro_amd import _lib as L
    P = oracle.default_params()
    ext = L.make_ext_bc(fill_ambient_bc=1, ambient_density=0.5, ambient_temp=3.0, ambient_energy=2.0)
    want = L.ambient_state(P, 0.5, 3.0, 2.0)
    once = L.complete_ext_bc(ext, P, -1.0)
    assert tuple(once.ambient_state) == want and once.const_grav == -1.0
    assert tuple(L.complete_ext_bc(once, P, 0.0).ambient_state) == want            # a completed struct completes to the same
    assert tuple(L.complete_ext_bc(ext.copy(), P, 0.0).ambient_state) == want
    small = L.ambient_state(P)
    for bare in (L.ExtBc(), L.ExtBc.from_buffer_copy(ext)):
        assert (bare.ambient_density, bare.ambient_temp, bare.ambient_energy) == (-1.e200,) * 3
        assert tuple(L.complete_ext_bc(bare, P, 0.0).ambient_state) == small
    assert bytes(ext.copy()) == bytes(ext)


def test_a_box_without_buffers_fills_without_a_counter(oracle):
    """Castro(alloc=False, ext_bc=...) -- the bookkeeping of a box another rank owns -- has no reduction buffer, so no counter:
    its boundary fill hands a null pointer on instead of failing"""
    import castro_amd
    n = (4, 4, 8)
    ext = castro_amd.make_ext_bc(zl="hse")
    c = castro_amd.Castro(n, params=oracle.default_params(), hydro=ExtBcOracleBackend(), ext_bc=ext, alloc=False, **ATMOS)
    assert c.ext_bc is not None and c._unconverged is None
    S = torch.from_numpy(_hse_atmosphere((n[0] + 8, n[1] + 8, n[2] + 8)))
    box = ((-4, -4, -4), (n[0] + 3, n[1] + 3, n[2] + 3))
    c._bc_fill_state(S, box)
    want = S.clone()
    c.hydro.bc_fill(want, box, c.geom)
    assert not torch.equal(S[:, :4], want[:, :4])                   # the hydrostatic walk has been there
    assert torch.equal(S[:, 4:-4, 4:-4, 4:-4], want[:, 4:-4, 4:-4, 4:-4])

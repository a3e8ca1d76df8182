"""GPU tests of the migration of tracer particles between ranks (castro_amd/csrc/tracer_kernels.hip: k_tracer_dest, k_tracer_scan,
k_tracer_pack, k_tracer_unpack; Castro / CastroAmr(tracers=..., comm=DistComm())), for both numerics builds.

Kernel level: integer work and bit copies, so destinations, counts, kept arrays and wire records equal the numpy restatement
(tests/tracer_migrate_ref.py) bit for bit.  Driver level: the two scenarios of tests/tracer_migrate_cases.py with 2 and 3
processes sharing the test GPU over gloo against the one-process run of the same build, bit for bit, files included -- the
multi-rank state equals the one-rank state bit for bit in both builds, so the particles do too: no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import tracer_migrate_cases as K
from tests import tracer_migrate_ref as M
from tests import tracer_ref as R
from tests import test_tracers_gpu as T

pytestmark = pytest.mark.gpu

CAP = 256                   # CASTRO_AMD_TRACER_MAX_RANKS
NS = (0, 1, 63, 64, 65, 256, 257, 1000)
SENTINEL = -7


@pytest.fixture(scope="module", params=["exact", "contract"])
def hydro(request):
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=request.param)
    yield h
    h.close()


def _owners(nranks):
    """level 0: one box per rank, box g owned by rank (g + 1) % nranks; level 1: two boxes of the last rank and of rank 0"""
    return [[(g + 1) % nranks for g in range(nranks)], [nranks - 1, 0]]


def _composition(kind, n, nranks, me, rng):
    """n particles whose destinations follow `kind`"""
    P = R.particles(rng.uniform(size=(n, 3)))
    P["r0"][:], P["r1"][:], P["r2"][:] = rng.normal(size=(3, n))
    P["cpu"][:] = rng.integers(0, 1 << 20, size=n)
    t = np.arange(n)
    other = (me + 1) % nranks
    if kind == "stay":
        dest = np.full(n, me)
    elif kind == "one":
        dest = np.full(n, other)
    elif kind == "wave":                                        # every destination inside one wave (64 of them at the cap)
        dest = t % nranks
    elif kind == "alternate":                                   # lane by lane
        dest = np.where(t % 2 == 0, me, other)
    else:
        dest = np.where(rng.uniform(size=n) < 0.8, me, rng.integers(0, nranks, size=n))
    P["grid"][:] = (dest - 1) % nranks                          # level 0: box g belongs to rank (g + 1) % nranks
    if kind in ("invalid", "outside"):
        second = rng.uniform(size=n) < 0.2                      # some on level 1
        P["level"][second] = 1
        P["grid"][second] = rng.integers(0, 2, size=int(second.sum()))
    if kind == "invalid":
        P["id"][t % 3 == 1] *= -1
    if kind == "outside":
        P["grid"][t % 5 == 0] = nranks + 3
        P["grid"][t % 7 == 0] = -1
        P["level"][t % 11 == 0] = 2
        P["level"][t % 13 == 0] = -1
        sel = (t % 17 == 0)
        P["level"][sel], P["grid"][sel] = 0, nranks             # no box of level 0, though the concatenated table has that entry
    return P


def _run(hydro, P, owners, nranks, me, pad=3):
    """(dest, counts, kept dict, wire) of the device; arrays padded with sentinels that must survive"""
    from castro_amd import _lib
    n = P["id"].shape[0]
    dev = T._device_particles(P)
    dest = torch.full((n + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    counts = torch.full((nranks + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    hydro.tracer_migrate_count(owners, nranks, me, dev[3], dest, counts)
    c = counts.tolist()
    assert c[nranks:] == [SENTINEL] * pad and dest[n:].tolist() == [SENTINEL] * pad
    nkeep, nleave = c[me], sum(c[:nranks]) - c[me]
    pos = torch.full((3, nkeep), float(SENTINEL), dtype=torch.float64, device="cuda")
    r = torch.full((3, nkeep), float(SENTINEL), dtype=torch.float64, device="cuda")
    ints = torch.full((4, nkeep), SENTINEL, dtype=torch.int32, device="cuda")
    wire = torch.full((nleave + pad, 8), SENTINEL, dtype=torch.int64, device="cuda")
    out = _lib.make_tracers(pos, r, ints)
    # the wire tensor is larger than the records: the call gets exactly nleave of it
    _lib.check(hydro.lib.castro_amd_tracer_migrate_pack(hydro.h, nranks, me, C.byref(dev[3]), C.c_void_p(dest.data_ptr()), C.byref(out),
                                                        C.c_void_p(wire.data_ptr()), nleave, None), "tracer_migrate_pack")
    torch.cuda.synchronize()
    T._same(dev, P, "the input arrays are not written")
    assert (wire[nleave:] == SENTINEL).all()
    pos, r, ints = pos.cpu().numpy(), r.cpu().numpy(), ints.cpu().numpy()
    kept = dict(x=pos[0], y=pos[1], z=pos[2], r0=r[0], r1=r[1], r2=r[2], id=ints[0], cpu=ints[1], level=ints[2], grid=ints[3])
    return dest[:n].cpu().numpy(), np.array(c[:nranks], dtype=np.int32), kept, wire[:nleave].cpu().numpy()


def _equal(P, Q, what):
    for k in M.REALS:
        assert np.array_equal(P[k].view(np.int64), Q[k].view(np.int64)), "%s: %s" % (what, k)
    for k in M.INTS:
        assert np.array_equal(P[k], Q[k]), "%s: %s" % (what, k)


@pytest.mark.parametrize("nranks", [2, 3, 8, CAP])
@pytest.mark.parametrize("n", NS)
def test_count_and_pack_bits(hydro, n, nranks):
    """N at the wave edge, the block edge and over four blocks (one trip of the scan over blocks, which takes 256 blocks a trip; two
    and three trips are tests/test_chunk_caps_gpu.py); 2, 3, 8 ranks and the cap; all stay, all leave to one rank, every
    destination inside one wave, destinations alternating lane by lane, a third invalid, grids and levels outside the table"""
    owners = _owners(nranks)
    for q, kind in enumerate(("stay", "one", "wave", "alternate", "invalid", "outside")):
        me = (q + nranks - 1) % nranks
        P = _composition(kind, n, nranks, me, np.random.default_rng(100 * n + nranks + q))
        want_dest, want_counts = M.destinations(P, owners, nranks, me)
        want_kept, want_wire = M.pack(P, want_dest, nranks, me)
        dest, counts, kept, wire = _run(hydro, P, owners, nranks, me)
        assert np.array_equal(dest, want_dest), kind
        assert np.array_equal(counts, want_counts), kind
        _equal(kept, want_kept, kind)
        assert np.array_equal(wire, want_wire), kind
        if n >= 63 and kind == "stay":
            assert counts[me] == n
        if n >= 63 and kind == "one":
            assert counts[me] == 0 and counts[(me + 1) % nranks] == n
        if n >= 63 and kind == "wave":
            assert (counts > 0).sum() == min(nranks, n)


def test_round_trip_into_arrays_that_hold_particles(hydro):
    """pack on rank a, unpack the records for rank b behind particles b already holds: [at, at + nrecv) are the arrivals,
    nothing else changes"""
    nranks, a, b = 3, 0, 2
    owners = _owners(nranks)
    P = _composition("mix", 700, nranks, a, np.random.default_rng(5))
    dest, counts, kept, wire = _run(hydro, P, owners, nranks, a)
    first = int(counts[1])                                      # the records for rank 1 come first
    nrecv = int(counts[b])
    assert nrecv > 10 and first > 10
    Q = _composition("stay", 300 + nrecv + 5, nranks, b, np.random.default_rng(6))
    dev = T._device_particles(Q)
    at = 300
    rec = torch.from_numpy(wire[first:first + nrecv].copy()).cuda()
    hydro.tracer_unpack(rec, dev[3], at)
    torch.cuda.synchronize()
    want = R.copy_particles(Q)
    M.unpack(wire[first:first + nrecv], want, at)
    T._same(dev, want, "unpack")
    sel = np.nonzero(dest == b)[0]
    for k in P:
        assert np.array_equal(want[k][at:at + nrecv], P[k][sel]), k                 # what left a is what arrived on b
        assert np.array_equal(want[k][:at], Q[k][:at]) and np.array_equal(want[k][at + nrecv:], Q[k][at + nrecv:])


def test_argument_checks(hydro):
    from castro_amd import _lib
    nranks, me, n = 3, 1, 200
    owners = _owners(nranks)
    P = _composition("mix", n, nranks, me, np.random.default_rng(8))
    dev = T._device_particles(P)
    dest = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    counts = torch.full((nranks,), SENTINEL, dtype=torch.int32, device="cuda")
    lib, h = hydro.lib, hydro.h
    cnt = (C.c_int * 2)(nranks, 2)
    own = (C.c_int * (nranks + 2))(*[o for ol in owners for o in ol])
    dp, cp = C.c_void_p(dest.data_ptr()), C.c_void_p(counts.data_ptr())

    def count(nlev=2, cnt=cnt, own=own, nranks=nranks, me=me, tr=dev[3], dp=dp, cp=cp):
        return lib.castro_amd_tracer_migrate_count(h, nlev, cnt, own, nranks, me, C.byref(tr) if tr is not None else None, dp, cp, None)
    assert count(tr=None) == _lib.ERR_ARG and count(cnt=None) == _lib.ERR_ARG and count(own=None) == _lib.ERR_ARG
    assert count(dp=None) == _lib.ERR_ARG and count(cp=None) == _lib.ERR_ARG
    assert count(me=-1) == _lib.ERR_ARG and count(me=nranks) == _lib.ERR_ARG
    assert count(nlev=0) == _lib.ERR_ARG and count(nlev=17) == _lib.ERR_ARG
    bad = (C.c_int * (nranks + 2))(*([0] * (nranks + 1) + [nranks]))                # an owner outside [0, nranks)
    assert count(own=bad) == _lib.ERR_ARG
    bad[nranks + 1] = -1
    assert count(own=bad) == _lib.ERR_ARG
    big = (C.c_int * (CAP + 3))(*([0] * (CAP + 3)))
    assert count(cnt=(C.c_int * 2)(CAP + 1, 2), own=big, nranks=CAP + 1) == _lib.ERR_UNSUPPORTED
    nul = _lib.Tracers.from_buffer_copy(dev[3])
    nul.level = None
    assert count(tr=nul) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert (dest == SENTINEL).all() and (counts == SENTINEL).all(), "a refused call writes nothing"

    # n == 0: OK, nothing launched, the counts are zero
    zero = T._device_particles(R.particles(np.zeros((0, 3))))
    assert count(tr=zero[3]) == _lib.OK
    assert counts.tolist() == [0] * nranks
    # the pack belongs to the count call before it: not to one of another n
    out_t = T._device_particles(R.particles(np.zeros((n, 3))))
    wire = torch.full((n, 8), SENTINEL, dtype=torch.int64, device="cuda")

    def pack(nranks=nranks, me=me, tr=dev[3], dp=dp, out=out_t[3], wp=C.c_void_p(wire.data_ptr()), nwire=n):
        return lib.castro_amd_tracer_migrate_pack(h, nranks, me, C.byref(tr) if tr is not None else None, dp,
                                                  C.byref(out) if out is not None else None, wp, nwire, None)
    assert pack() == _lib.ERR_ARG                                                   # the last count call had n == 0
    assert count() == _lib.OK
    assert pack(tr=None) == _lib.ERR_ARG and pack(out=None) == _lib.ERR_ARG and pack(dp=None) == _lib.ERR_ARG
    assert pack(wp=None) == _lib.ERR_ARG and pack(nwire=-1) == _lib.ERR_ARG
    assert pack(wp=C.c_void_p(wire.data_ptr() + 8)) == _lib.ERR_ARG                 # not 16-byte aligned
    assert pack(me=nranks) == _lib.ERR_ARG and pack(nranks=CAP + 1) == _lib.ERR_UNSUPPORTED
    assert pack(nranks=2, me=0) == _lib.ERR_ARG                                     # not the nranks of the count call
    assert pack(out=dev[3]) == _lib.ERR_ARG                                         # in place
    torch.cuda.synchronize()
    assert (wire == SENTINEL).all(), "a refused call writes nothing"
    T._same(out_t, R.particles(np.zeros((n, 3))), "a refused call writes nothing")

    def unpack(wp=C.c_void_p(wire.data_ptr()), nrecv=10, out=out_t[3], at=0):
        return lib.castro_amd_tracer_unpack(h, wp, nrecv, C.byref(out) if out is not None else None, at, None)
    assert unpack(wp=None) == _lib.ERR_ARG and unpack(out=None) == _lib.ERR_ARG and unpack(nrecv=-1) == _lib.ERR_ARG
    assert unpack(at=-1) == _lib.ERR_ARG and unpack(at=n - 9) == _lib.ERR_ARG and unpack(nrecv=n + 1) == _lib.ERR_ARG
    assert unpack(nrecv=0, at=n) == _lib.OK and unpack(nrecv=0, at=n + 1) == _lib.ERR_ARG
    torch.cuda.synchronize()
    T._same(out_t, R.particles(np.zeros((n, 3))), "a refused call writes nothing")


def test_boxes_without_a_fab_are_skipped_and_counted(hydro):
    """a table in which box 1 belongs to another rank: advect and sample skip its particles and add 1 to flags[0] for each,
    count drops them (it has no flags, as for a grid outside the table); everything else as in the call without them"""
    boxes, geom, dt, _ = T._level()
    P0 = T._case(1000)[0]
    theirs = (P0["id"] > 0) & (P0["level"] == 0) & (P0["grid"] == 1)
    nt = int(theirs.sum())
    assert nt > 50

    def without(P):                                             # the same particles, those of box 1 out of the level
        Q = dict(P)
        Q["level"] = np.where(theirs, -1, P["level"]).astype(np.int32)
        return Q
    fabs = [T._t(fab) for fab, _, _ in boxes]
    tab = hydro.make_tracer_boxes([(vb[0], vb[1], (f, ab) if i != 1 else None) for i, (f, (_, ab, vb)) in enumerate(zip(fabs, boxes))])
    P, dev = R.copy_particles(P0), T._device_particles(P0)
    flags, want_flags = torch.zeros(2, dtype=torch.int32, device="cuda"), np.zeros(2, dtype=np.int32)
    for ipass in (0, 1):
        hydro.tracer_advect(0, tab, geom, dt, ipass, dev[3], flags)
        R.advect_pass(without(P), 0, boxes, geom, dt, ipass, want_flags)
        torch.cuda.synchronize()
        T._same(dev, P, "advect pass %d" % ipass)
        assert flags.tolist() == [nt * (ipass + 1), 0] and not want_flags.any()
    for k in P:
        assert np.array_equal(P[k][theirs], P0[k][theirs])

    P, dev = R.copy_particles(P0), T._device_particles(P0)
    flags.zero_()
    out = torch.full((2, 1000), float(SENTINEL), dtype=torch.float64, device="cuda")
    want = np.full((2, 1000), float(SENTINEL))
    hydro.tracer_sample(0, tab, geom, (6, 0), dev[3], out, flags)
    R.sample(without(P), 0, boxes, geom, (6, 0), want, want_flags)
    assert np.array_equal(out.cpu().numpy().view(np.int64), want.view(np.int64)) and (want[:, theirs] == SENTINEL).all()
    assert flags.tolist() == [nt, 0] and not want_flags.any()

    cnt = [torch.zeros(tuple(vb[1][d] - vb[0][d] + 1 for d in (2, 1, 0)), dtype=torch.int32, device="cuda") for _, _, vb in boxes]
    ctab = hydro.make_tracer_boxes([(vb[0], vb[1], (c, vb) if i != 1 else None) for i, (c, (_, _, vb)) in enumerate(zip(cnt, boxes))])
    hydro.tracer_count(0, ctab, geom, dev[3])
    wcnt = [np.zeros(tuple(c.shape), dtype=np.int32) for c in cnt]
    R.count(without(P), 0, [(w, vb) for w, (_, _, vb) in zip(wcnt, boxes)], geom)
    torch.cuda.synchronize()
    for i in range(3):
        assert np.array_equal(cnt[i].cpu().numpy(), wcnt[i]), "count box %d" % i
    assert not wcnt[1].any() and wcnt[0].sum() > 0
    T._same(dev, P0, "sample and count write no particle")


# ---- driver level ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_process(hydro, tmp_path_factory):
    """the one-process runs of the build, made once: (case, world) -> (arrays, directory)"""
    cache = {}

    def get(case, world):
        key = (case, world if case == "single" else 0)
        if key not in cache:
            d = str(tmp_path_factory.mktemp("one_%s_%s" % (case, hydro.numerics)))
            cache[key] = (K.run(case, None, world, "hip", hydro.numerics, d), d)
            torch.cuda.synchronize()
        return cache[key]
    return get


@pytest.mark.parametrize("case,world", [("single", 2), ("single", 3), ("amr", 2), ("amr", 3)])
def test_processes_sharing_the_gpu_equal_one_process(hydro, one_process, tmp_path, case, world):
    """the scenarios of tests/test_tracer_migrate_cpu.py on the device: `world` processes share the GPU (gloo transport; RCCL
    needs a device per rank -- everything else is the code of a multi-GPU run: device count, pack, staged exchange, device
    unpack), compared with the one-process run of the same build bit for bit, files included; the same conditions against a
    vacuous pass.

    The AMR cases of the contract build are also the test that a level cleaned through an operation table (all boxes on one
    rank) and one cleaned box by box (boxes over ranks) give the same state bits: CASTRO_AMD_OP_CLEAN once ran a copy of
    clean_zone of its own, and one `r` entry of 600 came out 6.9e-18 off after the second coarse step."""
    import torch.multiprocessing as mp
    from tests.test_driver_cpu import _free_port
    d = str(tmp_path)
    mp.spawn(K.worker, args=(world, _free_port(), case, "hip", hydro.numerics, d), nprocs=world, join=True)
    one, one_dir = one_process(case, world)
    K.check(case, dict(np.load(os.path.join(d, "run.npz"))), one, world, d, one_dir)

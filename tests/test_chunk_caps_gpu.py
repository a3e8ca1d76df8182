"""GPU tests BEYOND THE FIRST CHUNK of the kernels and launchers that cut their work into pieces of a fixed size, for both numerics
builds: k_tracer_scan over more than 256 blocks (two and three trips), launch_clean_state_boxes with more than 32 regions (three
tables, skipped entries either side of a table boundary), group_chunks with more than 32 halo regions of one FAB (two and three
chunks of pack, unpack-local and unpack-remote), castro_amd_pack_regions_fab / castro_amd_unpack_regions_fab at their cap of 32,
and k_estdt / k_clean_state_reduce with the deciding zone in the last of three trips of their grid of 2048 workgroups.  The
shapes are those of tests/grid_caps.py, the smallest that cross each chunk (tests/test_grid_caps_cpu.py asserts that they do).

References: tests/tracer_migrate_ref.py (numpy) for the migration; castro_amd_clean_state_fab box by box and the oracle's
ora_clean_state for the tables of regions; a numpy gather through the periodic wrap for the halo exchange; numpy slicing for the
region tables; the oracle (`exact`) and the same kernel on one-trip slabs (both builds) for the reductions.  Everything is
compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import grid_caps as G
from tests import tracer_migrate_ref as M
from tests.test_gpu_parity import _ghosts_from_the_level, _to_dev
from tests.test_tracer_migrate_gpu import _composition, _equal, _owners, _run
from tests.util import physical_state, ulp_report

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


def _bits(t):
    return t.view(torch.int64)


# ---- 1. tracer migration over more than 256 blocks ------------------------------------------------------------------------------------
def _tracer_case(kind, n, nranks):
    """(me, particles, destinations, counts) of a composition; the destinations of the restatement are computed once"""
    q = G.TRACER_KINDS.index(kind)
    me = (q + nranks - 1) % nranks
    P = _composition(kind, n, nranks, me, np.random.default_rng(100 * n + nranks + q))
    key = ("tracer", kind, n, nranks)
    if key not in _CACHE:
        _CACHE[key] = M.destinations(P, _owners(nranks), nranks, me)
    return (me, P) + _CACHE[key]


def _check_migration(hydro, kind, n, nranks):
    me, P, want_dest, want_counts = _tracer_case(kind, n, nranks)
    want_kept, want_wire = M.pack(P, want_dest, nranks, me)
    dest, counts, kept, wire = _run(hydro, P, _owners(nranks), nranks, me)     # asserts that the sentinels behind every array survive
    assert np.array_equal(dest, want_dest), kind
    assert np.array_equal(counts, want_counts), kind
    _equal(kept, want_kept, kind)
    assert np.array_equal(wire, want_wire), kind
    return me, counts


@pytest.mark.parametrize("nranks", G.TRACER_RANKS)
@pytest.mark.parametrize("n", G.TRACER_NS)
def test_migration_over_more_than_one_trip_of_the_scan(hydro, n, nranks):
    """65 537 particles are 257 blocks, two trips of k_tracer_scan with one block in the second; 131 373 are 514 blocks, three
    trips, the last partial.  3 ranks and the cap of 256.  Destinations, counts, kept arrays and wire records equal the numpy
    restatement bit for bit, the sentinels behind every array survive.  With particles for every rank in every trip ("wave",
    "mix") three trips tell a carry that is assigned from one that is added."""
    assert G.scan_trips(n, 256, 256)[1] in (2, 3)
    for kind in G.TRACER_KINDS:
        me, counts = _check_migration(hydro, kind, n, nranks)
        if kind == "stay":
            assert counts[me] == n
        if kind == "one":
            assert counts[me] == 0 and counts[(me + 1) % nranks] == n
        if kind in G.TRACER_SPREAD:
            assert (counts > 0).sum() >= 2, kind
        if kind == "wave":
            assert (counts > 0).sum() == nranks and counts.min() >= n // nranks


@pytest.mark.parametrize("numerics", ["exact", "contract"])
def test_hist_workspace_grows_and_holds_a_smaller_table_again(numerics):
    """the hist workspace of one context (tr_migrate_scratch): 1000, then 131 373, then 1000 particles with 3 ranks, then the same
    with 256 -- the workspace grows, the row behind the last block moves, and stale larger contents lie behind a smaller table"""
    import castro_amd
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=numerics)
    try:
        for nranks in G.TRACER_RANKS:
            for n in G.TRACER_WORKSPACE_NS:
                me, counts = _check_migration(h, "mix", n, nranks)
                assert (counts > 0).sum() >= 2 and counts.sum() == n
    finally:
        h.close()


# ---- 2. more than 32 clean regions in one call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(G.CLEAN_CASES))
def test_clean_tables_beyond_one_launch(hydro, oracle, case):
    """OP_CLEAN operations through castro_amd_fab_ops_p on FABs of 3 x 2 x 4 valid zones: 70 that clean (three launches of
    k_clean_state: 32 + 32 + 6), exactly 32 and exactly 33, `ntimes` 1 and 2 mixed, with empty regions and `ntimes` 0 planted at
    positions 0, 31, 32, 33, 69, at the end and on either side of the entry that fills a table.  Equal to castro_amd_clean_state_fab
    box by box (one compiled copy of the sweep: both builds) and, in the `exact` build, to ora_clean_state; the FABs of the
    skipped operations keep their bits; one launch per 32 operations that clean."""
    import castro_amd
    from castro_amd import _lib as L
    kinds = G.clean_kinds(case)
    tables = G.clean_tables(kinds, 32)
    rng = np.random.default_rng(71)
    P = castro_amd.default_params(small_dens=0.3)
    ext, ng = G.CLEAN_FAB["valid"], G.CLEAN_FAB["ng"]
    host, many, one, specs, boxes = [], [], [], [], []
    for p, kind in enumerate(kinds):
        vlo = (p % 5 - 2, 3 - p % 4, p % 3)
        vhi = tuple(vlo[d] + ext[d] - 1 for d in range(3))
        fbox = (tuple(x - ng for x in vlo), tuple(x + ng for x in vhi))
        f = physical_state(rng, fbox[0], fbox[1], smooth=False)
        f[0] *= rng.uniform(0.2, 1.0, size=f[0].shape)              # some densities below small_dens, rho X != rho
        ntimes = 1 + p % 2
        lo, hi = vlo, vhi
        if kind == "empty":
            d = p % 3
            hi = tuple(lo[x] - 1 if x == d else hi[x] for x in range(3))
        if kind == "zero":
            ntimes = 0
        host.append(f)
        many.append(_to_dev(hydro, f))
        one.append(_to_dev(hydro, f))
        boxes.append((fbox, lo, hi, ntimes))
        specs.append((L.OP_CLEAN, 0, 8, lo, hi, float(ntimes), 0.0, (many[p], fbox), (many[p], fbox), None))
    assert {b[3] for b, k in zip(boxes, kinds) if k == "clean"} == {1, 2}
    for p, (fbox, lo, hi, ntimes) in enumerate(boxes):              # box by box
        if kinds[p] == "clean":
            hydro.clean_state(one[p], fbox, lo, hi, P, ntimes=ntimes)
    hydro.profile(True)
    hydro.profile_reset()
    try:
        hydro.fab_ops(hydro.make_ops(specs), params=P)
        torch.cuda.synchronize()
        launches = hydro.profile_report()["k_clean_state"][1]
    finally:
        hydro.profile(False)
    Po = oracle.default_params(small_dens=0.3)
    for p, (fbox, lo, hi, ntimes) in enumerate(boxes):
        if kinds[p] != "clean":
            assert np.array_equal(many[p].cpu().numpy().view(np.int64), host[p].view(np.int64)), "skipped operation %d (%s)" % (p, kinds[p])
            continue
        assert torch.equal(_bits(many[p]), _bits(one[p])), p
        got = many[p].cpu().numpy()
        assert not np.array_equal(got, host[p]), "cleaning changes values"
        if hydro.numerics == "exact":
            want = host[p].copy()
            for _ in range(ntimes):
                oracle.lib().ora_clean_state(oracle.i3(lo), oracle.i3(hi), oracle.a4(want, *fbox), C.byref(Po))
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), p
    assert launches == len(tables), "one launch of k_clean_state per 32 operations that clean: %d for %s" % (launches, [len(t) for t in tables])


# ---- 3. a FAB with more than 32 halo regions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_send", [0, 1])
@pytest.mark.parametrize("layout", sorted(G.HALO_PERIODIC))
def test_fill_boundary_group_with_more_regions_than_a_chunk(hydro, layout, self_send, monkeypatch):
    """one box of 8 x 16 x 16 facing sixteen boxes of 8 x 4 x 4 on one rank: FAB 0 sends and receives 32 (periodic in x: one full
    chunk, then an empty flush), 50 (x and z: 32 + 18) or 80 (x, y and z: 32 + 32 + 16) messages.  self_send 0: unpack-local
    chunks; 1: unpack-remote chunks through RCCL to the own rank.  Every ghost zone inside a box, or inside a periodic image of
    one, takes that box's valid data bit for bit; every other zone keeps its value."""
    from castro_amd import halo
    monkeypatch.setenv("CASTRO_AMD_HALO_SELF_SEND", str(self_send))
    boxes, ng, periodic = G.HALO_BOXES, G.HALO_NG, G.HALO_PERIODIC[layout]
    nb = len(boxes)
    local, sends, recvs = halo.level_messages(boxes, [0] * nb, 0, ng, G.HALO_DOMAIN, periodic)
    assert local == list(range(nb))
    assert sum(1 for m in sends if m[0] == 0) == sum(1 for m in recvs if m[0] == 0) == G.HALO_FAB0_MESSAGES[layout]
    gboxes = [(tuple(x - ng for x in lo), tuple(x + ng for x in hi)) for lo, hi in boxes]
    rng = np.random.default_rng(13)
    comm = hydro.comm_create(1, 0, hydro.comm_unique_id())
    try:
        for ncomp in (1, 8):
            group = hydro.halo_group(comm, nb, sends, recvs, ncomp)
            try:
                assert hydro.halo_group_bytes_sent(group) == (sum(8 * ncomp * G.zones(tuple(b[1][d] - b[0][d] + 1 for d in range(3)))
                                                                  for _, _, b, _ in sends) if self_send else 0)
                host = [rng.normal(size=(ncomp,) + tuple(g[1][d] - g[0][d] + 1 for d in (2, 1, 0))) for g in gboxes]
                dev = [_to_dev(hydro, a) for a in host]
                hydro.fill_boundary_group(group, dev, gboxes)
                torch.cuda.synchronize()
            finally:
                hydro.halo_group_destroy(group)
            for f, ((want, take), d) in enumerate(zip(_ghosts_from_the_level(boxes, host, ng, periodic), dev)):
                assert np.array_equal(d.cpu().numpy().view(np.int64), want.view(np.int64)), (ncomp, f)
                assert take.sum() > 0
    finally:
        hydro.comm_destroy(comm)


# ---- 4. pack_regions_fab / unpack_regions_fab directly -------------------------------------------------------------------------------------
SENT, SENT_FAB = -12345.0, 6789.5


def _region_fab(rng):
    lo, ext, ncomp = G.REGIONS_FAB["lo"], G.REGIONS_FAB["ext"], G.REGIONS_FAB["ncomp"]
    box = (lo, tuple(lo[d] + ext[d] - 1 for d in range(3)))
    return rng.normal(size=(ncomp, ext[2], ext[1], ext[0])), box


def _sl(box, lo, hi):
    return (slice(None),) + tuple(slice(lo[d] - box[0][d], hi[d] - box[0][d] + 1) for d in (2, 1, 0))


@pytest.mark.parametrize("empty", [(), G.REGIONS_EMPTY])
def test_pack_and_unpack_regions_at_the_cap(hydro, empty):
    """32 disjoint regions of one FAB of 13 x 11 x 9 zones at a negative `lo`, 8 components: whole cells, trimmed ones and slabs
    one zone thick, their slices handed out out of region order with gaps.  Pack against numpy slicing (component-major over the
    region, as k_pack), the gaps keep the sentinel; unpack into a sentinel-filled FAB changes the regions only; round trip.
    castro_amd_pack_regions_fab accepts an empty region (hi < lo): with regions 0, 15 and 31 emptied the others still land at
    their own offsets."""
    rng = np.random.default_rng(81)
    U, box = _region_fab(rng)
    ncomp = U.shape[0]
    boxes = G.regions()
    off, total = G.region_offsets(boxes, ncomp, empty)
    table_boxes = [((lo, tuple(lo[d] - 1 if d == r % 3 else hi[d] for d in range(3))) if r in empty else (lo, hi)) for r, (lo, hi) in enumerate(boxes)]
    table = hydro.region_table(table_boxes, off)
    live = [r for r in range(len(boxes)) if r not in empty]
    assert len(boxes) == 32 and len(live) == 32 - len(empty)

    def slices(a):                                              # region r of the FAB `a`, flattened as its slice of the buffer
        return {r: a[_sl(box, *boxes[r])].reshape(-1) for r in live}

    # pack
    Ud = _to_dev(hydro, U)
    buf = torch.full((total,), SENT, dtype=torch.float64, device=hydro.device)
    hydro.pack_regions(Ud, box, table, buf)
    torch.cuda.synchronize()
    want = np.full(total, SENT)
    for r, s in slices(U).items():
        assert np.all(want[off[r]:off[r] + s.size] == SENT), "the slices are disjoint"
        want[off[r]:off[r] + s.size] = s
    got = buf.cpu().numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), "the slices against numpy slicing, the gaps keep the sentinel"
    assert (want == SENT).sum() >= 32 and np.array_equal(Ud.cpu().numpy(), U), "pack does not write the FAB"
    # unpack another buffer into a sentinel-filled FAB: only the regions change
    B = rng.normal(size=total)
    V = torch.full(U.shape, SENT_FAB, dtype=torch.float64, device=hydro.device)
    Bd = _to_dev(hydro, B)
    hydro.unpack_regions(V, box, table, Bd)
    torch.cuda.synchronize()
    wantV = np.full(U.shape, SENT_FAB)
    for r in live:
        reg = wantV[_sl(box, *boxes[r])]
        reg[...] = B[off[r]:off[r] + reg.size].reshape(reg.shape)
    assert np.array_equal(V.cpu().numpy().view(np.int64), wantV.view(np.int64))
    assert (wantV == SENT_FAB).sum() > 0 and np.array_equal(Bd.cpu().numpy(), B), "unpack does not write the buffer"
    # round trip
    W = torch.full(U.shape, SENT_FAB, dtype=torch.float64, device=hydro.device)
    hydro.unpack_regions(W, box, table, buf)
    torch.cuda.synchronize()
    wantW = np.full(U.shape, SENT_FAB)
    for r in live:
        wantW[_sl(box, *boxes[r])] = U[_sl(box, *boxes[r])]
    assert np.array_equal(W.cpu().numpy().view(np.int64), wantW.view(np.int64))


def test_one_region_more_than_the_cap_is_refused(hydro, monkeypatch):
    """33 regions: castro_amd_pack_regions_fab and castro_amd_unpack_regions_fab refuse and write nothing; so does
    castro_amd_halo_plan_create, which takes 32"""
    rng = np.random.default_rng(82)
    U, box = _region_fab(rng)
    boxes = G.regions()
    lo, hi = boxes[0]
    assert hi[0] > lo[0]
    boxes = [(lo, (lo[0], hi[1], hi[2])), ((lo[0] + 1, lo[1], lo[2]), hi)] + boxes[1:]          # region 0 cut in two
    off, total = G.region_offsets(boxes, U.shape[0])
    table = hydro.region_table(boxes, off)
    assert table[0] == 33
    Ud = _to_dev(hydro, U)
    buf = torch.full((total,), SENT, dtype=torch.float64, device=hydro.device)
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.pack_regions(Ud, box, table, buf)
    with pytest.raises(RuntimeError, match="bad argument"):
        hydro.unpack_regions(Ud, box, table, buf)
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()) and np.array_equal(Ud.cpu().numpy(), U)
    hydro.pack_regions(Ud, box, hydro.region_table(boxes[:32], off[:32]), buf)          # the cap itself is taken
    torch.cuda.synchronize()
    assert not bool((buf == SENT).all())
    monkeypatch.setenv("CASTRO_AMD_HALO_SELF_SEND", "0")
    comm = hydro.comm_create(1, 0, hydro.comm_unique_id())
    try:
        regions = [(0, b, b, r, r) for r, b in enumerate(boxes)]
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.halo_plan(comm, regions, 8)
        hydro.halo_plan_destroy(hydro.halo_plan(comm, regions[:32], 8))
    finally:
        hydro.comm_destroy(comm)


# ---- 5. reductions with the deciding zone in the last trip -----------------------------------------------------------------------------------
GAMMA = 1.4
SMALL_DENS = 1.0e-2


def _reduce_state(name):
    """the state of a placement and the indices (in the FAB array) of its two planted zones.  The CFL zone moves at 100 in x (the
    others below 1); the density zone is its own state scaled to 0.05 (a tenth of the smallest other density), or to 1e-4, below
    small_dens.  Checked here with numpy: either zone wins by a wide margin, so no rounding decides the minimum."""
    if "reduce" not in _CACHE:
        c = G.REDUCE_BOX
        ng = c["ng"]
        glo = tuple(x - ng for x in c["lo"])
        ghi = tuple(c["lo"][d] + c["ext"][d] - 1 + ng for d in range(3))
        _CACHE["reduce"] = physical_state(np.random.default_rng(91), glo, ghi, jump=False)
    c, p = G.REDUCE_BOX, G.REDUCE_PLACEMENTS[name]
    ng, ext = c["ng"], c["ext"]
    U = _CACHE["reduce"].copy()
    zc = tuple(x + ng for x in p["cfl"])
    zr = tuple(x + ng for x in p["rho"])
    assert zc != zr
    rho = U[(0,) + zc]
    U[(1,) + zc] = 100.0 * rho
    U[(4,) + zc] = U[(5,) + zc] + 0.5 * (U[(1,) + zc] ** 2 + U[(2,) + zc] ** 2 + U[(3,) + zc] ** 2) / rho
    target = 1.0e-4 if p["below_small_dens"] else 0.05
    f = target / U[(0,) + zr]
    for n in (0, 1, 2, 3, 4, 5, 7):
        U[(n,) + zr] *= f
    assert (U[(0,) + zr] < SMALL_DENS) == p["below_small_dens"]
    # the margins, on the valid zones
    V = U[:, ng:-ng, ng:-ng, ng:-ng]
    assert V.shape[1:] == ext[::-1] and V[0].size > 2 * 524288
    dx = tuple(1.0 / e for e in ext)
    cs = np.sqrt(GAMMA * (GAMMA - 1.0) * V[5] / V[0])
    dt = np.minimum(np.minimum(dx[0] / (cs + np.abs(V[1] / V[0])), dx[1] / (cs + np.abs(V[2] / V[0]))), dx[2] / (cs + np.abs(V[3] / V[0])))
    rho = V[0].copy()
    assert np.unravel_index(np.argmin(dt), dt.shape) == p["cfl"] and np.unravel_index(np.argmin(rho), rho.shape) == p["rho"]
    best_dt, best_rho = dt[p["cfl"]], rho[p["rho"]]
    dt[p["cfl"]], rho[p["rho"]] = np.inf, np.inf
    assert 20.0 * best_dt < dt.min() and 5.0 * best_rho < rho.min(), (best_dt, dt.min(), best_rho, rho.min())
    return U, zc, zr


@pytest.mark.parametrize("placement", list(G.REDUCE_PLACEMENTS))
def test_reductions_with_the_deciding_zone_beyond_the_first_trip(hydro, oracle, placement):
    """128 x 64 x 130 zones at a non-zero `lo` in a FAB of four ghost zones: 8192 zones a k-plane, so the 2048 workgroups of k_estdt
    and k_clean_state_reduce take the planes [0, 64), [64, 128) and [128, 130) on their first, second and third trip.  The zone
    that decides the CFL estimate and the one of the smallest raw density lie in the last and the second trip, both in the first
    (the control), or in the first zone of the second trip and the very last zone of the box (there below small_dens).
    Both builds: the capped launch gives the state bits and the minima of the same kernel run on the three slabs, one trip each.
    `exact`: the cleaned state and red[0], red[1], red[2] equal the oracle bit for bit."""
    import castro_amd
    c = G.REDUCE_BOX
    lo, ext, ng = c["lo"], c["ext"], c["ng"]
    hi = tuple(lo[d] + ext[d] - 1 for d in range(3))
    box = (tuple(x - ng for x in lo), tuple(x + ng for x in hi))
    assert G.zones(ext) > 2 * 524288
    U, zc, zr = _reduce_state(placement)
    Ph = castro_amd.default_params(small_dens=SMALL_DENS)
    Gh = castro_amd.make_geom(ext, domlo=lo)
    assert Ph.eos_gamma == GAMMA
    slabs = [((lo[0], lo[1], lo[2] + a), (hi[0], hi[1], lo[2] + b - 1)) for a, b in G.REDUCE_SLABS]
    raw = _to_dev(hydro, U)

    def red(n):
        return torch.full((n,), 1e200, dtype=torch.float64, device=hydro.device)

    def estdt(state, what):
        whole, parts = red(2), [red(2) for _ in slabs]
        hydro.estdt_cfl(state, box, lo, hi, Gh, Ph, whole)
        for (slo, shi), r in zip(slabs, parts):
            hydro.estdt_cfl(state, box, slo, shi, Gh, Ph, r)
        torch.cuda.synchronize()
        assert torch.equal(_bits(whole), _bits(torch.stack(parts).amin(dim=0))), (what, whole.tolist(), [r.tolist() for r in parts])
        return whole.tolist()

    est_raw = estdt(raw, "estdt of the raw state")
    assert est_raw[1] == U[(0,) + zr], "the smallest density is the planted one"
    if hydro.numerics == "exact":
        Po = oracle.default_params(small_dens=SMALL_DENS)
        Go = oracle.make_geom(ext, domlo=lo)
        o3, a4 = oracle.i3, oracle.a4
        raw_min = oracle.lib().ora_min_density(o3(lo), o3(hi), a4(U, *box))
        assert raw_min == U[(0,) + zr]
        Uo, est_o = U.copy(), {}
    for ntimes in (1, 2):
        whole, parts = red(3), [red(3) for _ in slabs]
        S, T = raw.clone(), raw.clone()
        hydro.clean_state_reduce(S, box, lo, hi, Gh, Ph, whole, ntimes=ntimes)
        for (slo, shi), r in zip(slabs, parts):
            hydro.clean_state_reduce(T, box, slo, shi, Gh, Ph, r, ntimes=ntimes)
        torch.cuda.synchronize()
        assert torch.equal(_bits(S), _bits(T)), "ntimes %d: the state of the capped launch against the three slabs" % ntimes
        assert not torch.equal(_bits(S), _bits(raw)), "cleaning changes values"
        assert torch.equal(_bits(whole), _bits(torch.stack(parts).amin(dim=0))), (ntimes, whole.tolist(), [r.tolist() for r in parts])
        w = whole.tolist()
        assert w[1] == U[(0,) + zr], "red[1]: the smallest RAW density"
        est_clean = estdt(S, "estdt of the cleaned state")
        if hydro.numerics == "exact":
            oracle.lib().ora_clean_state(o3(lo), o3(hi), a4(Uo, *box), C.byref(Po))             # Uo: cleaned `ntimes` times
            est_o[ntimes] = oracle.lib().ora_estdt_cfl(o3(lo), o3(hi), a4(Uo, *box), C.byref(Go), C.byref(Po))
            ne, ad, rd = ulp_report(S.cpu().numpy(), Uo)
            assert ne == 0, "clean_state_reduce x%d: %d differ (max rel %.3e)" % (ntimes, ne, rd)
            assert w[0] == est_o[ntimes] and w[1] == raw_min and w[2] == est_o[1], (w, est_o, raw_min)
            assert est_clean[0] == est_o[ntimes] and est_clean[1] == oracle.lib().ora_min_density(o3(lo), o3(hi), a4(Uo, *box))

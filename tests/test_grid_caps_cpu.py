"""CPU guard of the GPU tests that cross the grid caps (tests/grid_caps.py): the caps, the workgroup sizes and the starting `iters`
are read out of the kernel sources and the header, and every shape the GPU tests use must cross its cap -- by the number of trips
stated here.  Raising a cap fails this test instead of leaving the GPU tests below it.  The same for the chunk sizes (the trips of
k_tracer_scan, CLEAN_BOXES_MAX, CASTRO_AMD_MAX_REGIONS, the 2048 workgroups of launch_estdt and launch_clean_state_reduce) and the
shapes of tests/test_chunk_caps_gpu.py."""
import os
import re

from tests import grid_caps as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "castro_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _const(src, name):
    m = re.findall(r"constexpr int %s = (\d+);" % name, src)
    assert len(m) == 1, name
    return int(m[0])


def _layout_loop(src, func):
    """(the starting iters, the largest iters) of the doubling loop of the layout function `func`"""
    body = src[src.index(func):]
    start = re.search(r"for \(iters = (\d+); ; iters \*= 2\)", body)
    stop = re.search(r"iters >= (\(1 << \d+\)|\d+)", body)
    assert start and stop and start.start() < stop.start() < 2500, func
    top = stop.group(1)
    return int(start.group(1)), (1 << int(top[6:-1]) if top.startswith("(") else int(top))


def _define(name):
    hdr = open(os.path.join(ROOT, "include", "castro_hydro_amd.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, hdr).group(1))


def test_every_shape_of_the_grid_cap_tests_crosses_its_cap():
    poisson, diag, pack = _src("poisson_kernels.hip"), _src("diag_kernels.hip"), _src("checkpoint_kernels.hip")
    max_bottom, max_order = _define("CASTRO_AMD_POISSON_MAX_BOTTOM"), _define("CASTRO_AMD_MAX_MULTIPOLE")

    # the norm: a grid-stride loop of two trips, and k_mg_norm_final reads every one of its rows
    wg, cap = _const(poisson, "MG_WG"), _const(poisson, "MG_NORM_MAX_WG")
    assert "for (long q = (long)blockIdx.x * MG_WG + threadIdx.x; q < total; q += (long)gridDim.x * MG_WG)" in poisson
    for n in (G.MG_NORM_ONE_BOX, G.bounding_extents(G.MG_NORM_UNION)):
        nb, want, trips = G.norm_layout(G.zones(n), wg, cap)
        assert (nb, trips) == (cap, 2) and want == 1280 > cap, (n, nb, want, trips)
        assert cap * wg == 64 * 64 * 64, "the zones of the second trip are those with k >= 64: the tests plant their values there"
    assert G.coarsened(G.MG_NORM_ONE_BOX)[-1] == (4, 4, 5) and G.zones((4, 4, 5)) <= max_bottom
    covered = sum(G.zones(tuple(b[1][d] - b[0][d] + 1 for d in range(3))) for b in G.MG_NORM_UNION)
    assert covered * 5 == G.zones(G.bounding_extents(G.MG_NORM_UNION)) * 4

    # the bottom solve: one workgroup, more than one trip per colour
    bwg = _const(poisson, "MG_BOTTOM_WG")
    assert "for (long q = threadIdx.x; q < nq; q += MG_BOTTOM_WG)" in poisson
    bottoms = [G.coarsened(n)[-1] for n in G.BOTTOM_ONE_BOX]
    assert bottoms == [(15, 16, 17), (13, 14, 15)]
    assert [G.bottom_trips(b, bwg) for b in bottoms] == [3, 2]
    ub = G.coarsened(G.bounding_extents(G.BOTTOM_UNION), G.alignment_levels(G.BOTTOM_UNION))
    assert ub == [(30, 32, 34), (15, 16, 17)] and G.bottom_trips(ub[-1], bwg) == 3
    assert all(G.zones(b) <= max_bottom for b in bottoms + [ub[-1]])
    assert G.bottom_trips((16, 16, 16), bwg) == 2 and max_bottom == 4096, "the largest bottom the plan accepts takes two trips"

    # the moments: iters = 2, half the workgroups; and the order cap
    mwg, mcap = _const(poisson, "MP_WG"), _const(poisson, "MP_MAX_WG")
    it0, top = _layout_loop(poisson, "static int mp_layout(")
    assert G.capped_layout(G.mp_box_zones(), mwg, mcap, it0, top) == (2, 576, 1152) and it0 == 1 and mcap < 1152
    assert sum(G.mp_box_zones()) == 294912 and G.MP_LARGE["lnum"] + 1 <= max_order + 1
    assert G.MP_ORDER == max_order
    assert _const(poisson, "MP_FINAL_GROUPS") * 2 * (max_order + 1) <= _const(poisson, "MP_FINAL_WG")

    # the integrated quantities: iters = 8
    dwg, dcap = _const(diag, "DIAG_WG"), _const(diag, "DIAG_MAX_WG")
    it0, top = _layout_loop(diag, "int diag_layout(")
    pairs = G.diag_pairs()
    assert pairs == 128 * 128 * 130 == 2129920
    iters, nb, first = G.capped_layout([pairs], dwg, dcap, it0, top)
    assert (it0, iters, nb, first) == (4, 8, 1040, 2080) and first > dcap and nb * dwg * it0 < pairs

    # pack, min / max, unpack: iters = 8 for each entry alone, 16 for both in one call
    pwg, pcap = _const(pack, "PACK_WG"), _const(pack, "PACK_MAX_WG")
    it0, top = _layout_loop(pack, "static int pack_layout(")
    assert not G.pack_vec2(G.PACK_ONE_ZONE) and G.pack_vec2(G.PACK_VEC2)
    assert G.pack_vec2(G.PACK_VEC2, offset=G.zones(G.PACK_ONE_ZONE["ext"]) * G.PACK_ONE_ZONE["ncomp"]), "the second entry of the pair keeps two zones per access"
    assert G.pack_units([G.PACK_ONE_ZONE])[0] == 552960 and G.pack_units([G.PACK_VEC2])[0] == 589824
    assert it0 == 4
    assert G.capped_layout(G.pack_units([G.PACK_ONE_ZONE]), pwg, pcap, it0, top) == (8, 2160, 4320)
    assert G.capped_layout(G.pack_units([G.PACK_VEC2]), pwg, pcap, it0, top) == (8, 2304, 4608)
    assert G.capped_layout(G.pack_units([G.PACK_ONE_ZONE, G.PACK_VEC2]), pwg, pcap, it0, top) == (16, 2232, 8928)
    assert pcap < 4320


# ---- the chunk sizes (tests/test_chunk_caps_gpu.py) -----------------------------------------------------------------------------------
def _body(src, head, length=2500):
    at = src.index(head)
    return src[at:at + length]


def test_tracer_counts_cross_the_trips_of_the_scan():
    tracer = _src("tracer_kernels.hip")
    scan = _body(tracer, "k_tracer_scan(int* __restrict__ hist")
    assert "for (long base = 0; base < nblocks; base += 256) {" in scan and "carry += s[255];" in scan
    assert "const long nb = (n + 255) / 256;" in _body(tracer, "static inline bool tr_grid(", 300), "blocks of 256 particles"
    assert [G.scan_trips(n, 256, 256) for n in G.TRACER_NS] == [(257, 2, 1), (514, 3, 2)]
    assert G.scan_trips(1000, 256, 256) == (4, 1, 4), "the four blocks of tests/test_tracer_migrate_gpu.py are one trip"
    assert max(G.TRACER_RANKS) == _define("CASTRO_AMD_TRACER_MAX_RANKS")
    assert G.TRACER_WORKSPACE_NS[1] == G.TRACER_NS[1] and G.scan_trips(G.TRACER_WORKSPACE_NS[0], 256, 256)[0] < 256
    assert set(G.TRACER_SPREAD) <= set(G.TRACER_KINDS)


def test_clean_cases_fill_more_than_two_tables():
    aux = _src("aux_kernels.hip")
    m = re.findall(r"#define CLEAN_BOXES_MAX (\d+)", aux)
    assert len(m) == 1
    cap = int(m[0])
    assert "for (; done < nbox && T.n < CLEAN_BOXES_MAX; ++done) {" in aux
    assert "if (n <= 0 || ntimes[done] <= 0) continue;" in aux
    kinds = G.clean_kinds("seventy")
    tables = G.clean_tables(kinds, cap)
    assert kinds.count("clean") == 70 > 2 * cap and [len(t) for t in tables] == [cap, cap, 70 - 2 * cap]
    for p in (0, 31, 32, 33, 69, len(kinds) - 1):
        assert kinds[p] != "clean", p
    for t in tables[:-1]:                                        # a skipped entry either side of the entry that fills a table
        assert kinds[t[-1] - 1] != "clean" and kinds[t[-1] + 1] != "clean", t[-1]
    run = [p for p in range(tables[0][-1] - 2, tables[0][-1] + 3) if kinds[p] != "clean"]
    assert len(run) == 3, "three skipped entries across the 32nd cleaning operation"
    assert {kinds[p] for t in tables[:-1] for p in (t[-1] - 1, t[-1] + 1)} == {"empty", "zero"}
    # exactly one table, and one region more; an operation of ntimes 0 that is not skipped would open a second launch of the first
    kinds = G.clean_kinds("thirty_two")
    assert [len(t) for t in G.clean_tables(kinds, cap)] == [cap] and "zero" in kinds
    assert len(G.clean_tables(["clean" if k == "zero" else k for k in kinds], cap)) == 2
    kinds = G.clean_kinds("thirty_three")
    tables = G.clean_tables(kinds, cap)
    assert [len(t) for t in tables] == [cap, 1]
    assert kinds[tables[0][-1] - 1] != "clean" and kinds[tables[0][-1] + 1] != "clean"


def test_halo_layouts_and_region_tables_cross_the_region_cap():
    from castro_amd import halo
    cap = _define("CASTRO_AMD_MAX_REGIONS")
    rccl = _src("halo_rccl.hip")
    assert "if ((int)c.off.size() == CASTRO_AMD_MAX_REGIONS) flush();" in rccl
    assert "nregions > CASTRO_AMD_MAX_REGIONS" in _body(rccl, "int castro_amd_halo_plan_create(", 600)
    assert "nregions > CASTRO_AMD_MAX_REGIONS" in _body(_src("capi.hip"), "static int pack_regions(", 600)
    # the boxes tile the domain
    assert sum(G.zones(tuple(b[1][d] - b[0][d] + 1 for d in range(3))) for b in G.HALO_BOXES) == 16 ** 3 and len(G.HALO_BOXES) == 17
    for name, periodic in G.HALO_PERIODIC.items():
        local, sends, recvs = halo.level_messages(G.HALO_BOXES, [0] * 17, 0, G.HALO_NG, G.HALO_DOMAIN, periodic)
        ns, nr = sum(1 for m in sends if m[0] == 0), sum(1 for m in recvs if m[0] == 0)
        assert ns == nr == G.HALO_FAB0_MESSAGES[name], (name, ns, nr)
        assert G.chunk_sizes(ns, cap) == G.HALO_FAB0_CHUNKS[name], name
        assert all(sum(1 for m in sends if m[0] == f) < cap for f in range(1, 17)), "only FAB 0 is cut into chunks"
    assert G.HALO_FAB0_MESSAGES == {"x": cap, "xz": 50, "xyz": 80}
    # the region table of the direct pack / unpack test: exactly the cap, disjoint, inside the FAB
    boxes = G.regions()
    lo0, ext = G.REGIONS_FAB["lo"], G.REGIONS_FAB["ext"]
    assert len(boxes) == cap and max(G.REGIONS_EMPTY) == cap - 1 and min(G.REGIONS_EMPTY) == 0
    seen = set()
    for lo, hi in boxes:
        assert all(lo0[d] <= lo[d] <= hi[d] < lo0[d] + ext[d] for d in range(3))
        z = {(i, j, k) for i in range(lo[0], hi[0] + 1) for j in range(lo[1], hi[1] + 1) for k in range(lo[2], hi[2] + 1)}
        assert not (z & seen)
        seen |= z
    assert any(min(hi[d] - lo[d] for d in range(3)) == 0 for lo, hi in boxes), "some are one zone thick"
    off, total = G.region_offsets(boxes, 8, G.REGIONS_EMPTY)
    assert off != sorted(off) and len(set(off)) == cap, "offsets out of region order"


def test_reduce_box_takes_three_trips_on_k_planes():
    aux = _src("aux_kernels.hip")
    for launcher, kernel in (("int launch_clean_state_reduce(", "k_clean_state_reduce"), ("int launch_estdt(", "k_estdt")):
        body = _body(aux, launcher, 900)
        assert "long nb = (n + 255) / 256;" in body and "if (nb > 2048) nb = 2048;" in body, launcher
        assert "hipLaunchKernelGGL(%s, dim3((unsigned)nb), dim3(256)" % kernel in body, launcher
        assert "tid < total; tid += (long)gridDim.x * blockDim.x) {" in _body(aux, "__global__ void __launch_bounds__(256) %s(" % kernel, 900)
    ext = G.REDUCE_BOX["ext"]
    per, trips, planes = G.reduce_trips(ext, 256, 2048)
    assert (per, trips, planes) == (524288, 3, [0, 64, 128]) and G.zones(ext) > 2 * per
    assert [s[0] for s in G.REDUCE_SLABS] == planes and G.REDUCE_SLABS[-1][1] == ext[2]
    assert all((b - a) * ext[0] * ext[1] <= per for a, b in G.REDUCE_SLABS), "a slab alone is one trip"
    trip_of = lambda k: max(t for t in range(trips) if planes[t] <= k)
    P = G.REDUCE_PLACEMENTS
    assert (trip_of(P["last_trip"]["cfl"][0]), trip_of(P["last_trip"]["rho"][0])) == (2, 1)
    assert (trip_of(P["control"]["cfl"][0]), trip_of(P["control"]["rho"][0])) == (0, 0)
    assert P["edges"]["cfl"] == (planes[1], 0, 0) and P["edges"]["rho"] == (ext[2] - 1, ext[1] - 1, ext[0] - 1)

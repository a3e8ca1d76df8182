"""CPU guard of the GPU tests that cross the grid caps (tests/grid_caps.py): the caps, the workgroup sizes and the starting `iters`
are read out of the kernel sources and the header, and every shape the GPU tests use must cross its cap -- by the number of trips
stated here.  Raising a cap fails this test instead of leaving the GPU tests below it."""
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

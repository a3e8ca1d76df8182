"""The shapes at which the tests cross the grid caps of the reduction and bottom-solve kernels, in one place (tests only): the GPU
tests import them, and tests/test_grid_caps_cpu.py reads the caps out of the kernel sources and asserts that every shape still
crosses its cap, and by how many trips -- a cap that is raised later fails that test instead of leaving the GPU tests below it.

The layout functions restate the launchers (launch_mg_norm, k_mg_bottom's loop, mp_layout, diag_layout, pack_layout) with the caps
as arguments; nothing here imports the product, torch or numpy.

The second half holds the shapes that cross the CHUNK sizes -- work cut into pieces of a fixed size instead of a capped grid:
the trips of k_tracer_scan, the tables of launch_clean_state_boxes, the chunks of group_chunks, the region tables of
castro_amd_pack_regions_fab and the trips of k_estdt / k_clean_state_reduce (tests/test_chunk_caps_gpu.py)."""

# ---- multigrid norm: more than MG_NORM_MAX_WG workgroups of MG_WG zones on level 0 ---------------------------------------------------
MG_NORM_ONE_BOX = (64, 64, 80)                                   # 327 680 zones; coarsens to (4, 4, 5)
MG_NORM_UNION = [((0, 0, 0), (63, 63, 47)), ((0, 0, 48), (31, 63, 79))]      # bounding box 64 x 64 x 80, 80 % covered

# ---- bottom solves of more than MG_BOTTOM_WG pairs -----------------------------------------------------------------------------------
BOTTOM_ONE_BOX = [(15, 16, 17), (26, 28, 30)]                    # the bottoms (15, 16, 17) and (13, 14, 15): 3 and 2 trips per colour
BOTTOM_UNION = [((2, 2, 2), (31, 33, 19)), ((2, 2, 20), (17, 33, 35))]       # aligned to 2 only: the bottom is level 1, 15 x 16 x 17
BOTTOM_UNION_CRSE_BOX = ((-1, -1, -1), (18, 18, 19))

# ---- multipole moments: more than MP_MAX_WG workgroups per order, and the order cap ---------------------------------------------------
MP_LARGE = dict(n_cell=(72, 64, 64), prob_hi=(4.5, 4.0, 4.0), center=(1.3, 2.2, 1.9), lnum=2,
                cuts=((0, 6), (7, 50), (51, 71)), ghosts=(1, 4, 3))
MP_ORDER = 16

# ---- integrated quantities: more than DIAG_MAX_WG workgroups at the starting iters ---------------------------------------------------
DIAG_LARGE = dict(n_cell=(256, 128, 256), lo=(1, 0, 0), ext=(255, 128, 130), ng=4)

# ---- pack / min-max / unpack: more than PACK_MAX_WG workgroups at the starting iters --------------------------------------------------
PACK_ONE_ZONE = dict(lo=(5, -3, 11), ext=(96, 80, 72), ng=3, ncomp=8)        # an odd ghost width: rows off the 16-byte grid
PACK_VEC2 = dict(lo=(-16, 8, 32), ext=(128, 96, 96), ng=4, ncomp=8)          # even everything: two zones per access


def zones(n):
    return n[0] * n[1] * n[2]


def ceil_div(a, b):
    return (a + b - 1) // b


def coarsened(n, align_levels=None):
    """the extents of the multigrid levels below n: halved while every extent is even and the half is at least 2 (and, for a
    union of boxes, for at most `align_levels` levels)"""
    out = [tuple(n)]
    while all(x % 2 == 0 and x // 2 >= 2 for x in out[-1]) and (align_levels is None or len(out) < align_levels):
        out.append(tuple(x // 2 for x in out[-1]))
    return out


def bounding_extents(boxes):
    return tuple(max(b[1][d] for b in boxes) - min(b[0][d] for b in boxes) + 1 for d in range(3))


def alignment_levels(boxes):
    """the levels the alignment of the boxes of a union allows: level m exists while every lo and hi + 1 is divisible by 2^m"""
    m = 1
    while all(b[0][d] % (1 << m) == 0 and (b[1][d] + 1) % (1 << m) == 0 for b in boxes for d in range(3)):
        m += 1
    return m


def norm_layout(nzones, wg, max_wg):
    """launch_mg_norm: (workgroups launched, workgroups an uncapped grid would have, most trips of a thread)"""
    want = ceil_div(nzones, wg)
    nb = min(want, max_wg)
    return nb, want, ceil_div(nzones, nb * wg)


def bottom_trips(n, wg):
    """k_mg_bottom: trips of thread 0 through the x-pairs of one colour of the level n"""
    return ceil_div(((n[0] + 1) // 2) * n[1] * n[2], wg)


def capped_layout(units, wg, max_wg, iters0, iters_max):
    """mp_layout / diag_layout / pack_layout: iters doubles from iters0 until the workgroups of all the stretches `units` (each
    rounded up on its own) fit under max_wg.  (iters, workgroups, workgroups at iters0)"""
    first = None
    iters = iters0
    while True:
        tot = sum(ceil_div(u, wg * iters) for u in units)
        if first is None:
            first = tot
        if tot <= max_wg or iters >= iters_max:
            return iters, tot, first
        iters *= 2


def mp_box_zones(case=MP_LARGE):
    n = case["n_cell"]
    return [(x1 - x0 + 1) * n[1] * n[2] for x0, x1 in case["cuts"]]


def diag_pairs(case=DIAG_LARGE):
    """diag_layout's units of a box in a FAB with `ng` ghost zones: with an odd row stride the rows start on either parity, and
    a row takes (n0 + 2) / 2 pairs; with even strides the parity of the first valid zone decides (a tensor's storage starts on
    a 16-byte boundary)"""
    ext, ng = case["ext"], case["ng"]
    sy, sz = ext[0] + 2 * ng, (ext[0] + 2 * ng) * (ext[1] + 2 * ng)
    shift = (ng & 1) if (sy % 2 == 0 and sz % 2 == 0) else 1
    return ((ext[0] + shift + 1) // 2) * ext[1] * ext[2]


def pack_vec2(entry, offset=0):
    """pack_table's rule for two zones per access: the first valid zone, the strides, the row length and the offset in the
    buffer all even (tensor and buffer start on 16-byte boundaries)"""
    ext, ng = entry["ext"], entry["ng"]
    sy = ext[0] + 2 * ng
    sz = sy * (ext[1] + 2 * ng)
    sn = sz * (ext[2] + 2 * ng)
    first = ng + sy * ng + sz * ng
    return all(v % 2 == 0 for v in (first, ext[0], sy, sz, sn, offset))


def pack_units(entries):
    """the stretches of pack_layout: one per (entry, component), items = zones or pairs of zones"""
    out, offset = [], 0
    for e in entries:
        z = zones(e["ext"])
        out += [z // 2 if pack_vec2(e, offset) else z] * e["ncomp"]
        offset += z * e["ncomp"]
    return out


# ======================================================================================================================================
# Chunk sizes: work cut into fixed-size pieces instead of a capped grid (tests/test_chunk_caps_gpu.py)
# ======================================================================================================================================

# ---- tracer migration: k_tracer_scan takes the blocks of 256 particles in trips of 256 ------------------------------------------------
TRACER_NS = (65537, 131073 + 300)                                # 257 blocks: two trips, the second of one block; 514: three trips
TRACER_RANKS = (3, 256)
TRACER_KINDS = ("stay", "one", "wave", "invalid", "outside", "mix")
TRACER_SPREAD = ("wave", "mix")                                  # particles for every rank in every trip
TRACER_WORKSPACE_NS = (1000, 131073 + 300, 1000)                 # the hist workspace grows, then holds a smaller table in front of stale rows

# ---- clean_state of many regions: one launch per CLEAN_BOXES_MAX non-empty regions -----------------------------------------------------
# (number of operations, {position: how it is skipped}): "empty" = hi < lo in one direction, "zero" = ntimes 0
CLEAN_FAB = dict(valid=(3, 2, 4), ng=2)
CLEAN_CASES = {
    # 70 cleaning operations and 11 skipped ones among them: at positions 0, 31, 32, 33 and 69, either side of the 32nd and of the 64th
    # cleaning operation (positions 36 and 72: the last entries of the first and the second table), and at the end
    "seventy": (81, {0: "empty", 31: "zero", 32: "empty", 33: "zero", 35: "empty", 37: "zero", 38: "empty", 69: "zero", 71: "zero",
                     73: "empty", 80: "zero"}),
    "thirty_two": (35, {0: "empty", 5: "zero", 34: "zero"}),      # one full table; an unskipped ntimes 0 would open a second
    "thirty_three": (37, {0: "zero", 17: "empty", 33: "zero", 35: "empty"}),   # positions 34 and 36: the 32nd and 33rd cleaning operation
}

# ---- halo groups: the regions of a FAB in chunks of CASTRO_AMD_MAX_REGIONS ---------------------------------------------------------------
HALO_DOMAIN = ((0, 0, 0), (15, 15, 15))
HALO_NG = 4
HALO_BOXES = [((0, 0, 0), (7, 15, 15))] + [((8, j, k), (15, j + 3, k + 3)) for k in (0, 4, 8, 12) for j in (0, 4, 8, 12)]
HALO_PERIODIC = {"x": (True, False, False), "xz": (True, False, True), "xyz": (True, True, True)}
HALO_FAB0_MESSAGES = {"x": 32, "xz": 50, "xyz": 80}            # sends = receives of FAB 0
HALO_FAB0_CHUNKS = {"x": [32], "xz": [32, 18], "xyz": [32, 32, 16]}

# ---- pack_regions_fab / unpack_regions_fab at the cap ---------------------------------------------------------------------------------
REGIONS_FAB = dict(lo=(-5, -3, -7), ext=(13, 11, 9), ncomp=8)
REGIONS_CUTS = ((0, 3, 6, 10, 13), (0, 2, 5, 8, 11), (0, 4, 9))  # 4 x 4 x 2 cells, one region inside each
REGIONS_EMPTY = (0, 15, 31)

# ---- k_estdt / k_clean_state_reduce: 2048 workgroups of 256 zones a trip ---------------------------------------------------------------
REDUCE_BOX = dict(lo=(3, -2, 5), ext=(128, 64, 130), ng=4)
REDUCE_SLABS = ((0, 64), (64, 128), (128, 130))                   # k-planes of the three trips, relative to lo
# (k-plane, j, i) relative to lo of the zone that decides the CFL estimate and of the one with the smallest raw density
REDUCE_PLACEMENTS = {
    "last_trip": dict(cfl=(129, 17, 41), rho=(100, 50, 7), below_small_dens=False),
    "control": dict(cfl=(3, 17, 41), rho=(3, 50, 7), below_small_dens=False),
    "edges": dict(cfl=(64, 0, 0), rho=(129, 63, 127), below_small_dens=True),
}


def scan_trips(n, block, trip):
    """k_tracer_dest / k_tracer_scan: (blocks of `block` particles, trips of `trip` blocks, blocks of the last trip)"""
    blocks = ceil_div(n, block)
    trips = ceil_div(blocks, trip)
    return blocks, trips, blocks - (trips - 1) * trip


def clean_kinds(case):
    """per position "clean", "empty" or "zero" """
    total, skipped = CLEAN_CASES[case]
    return [skipped.get(p, "clean") for p in range(total)]


def clean_tables(kinds, cap):
    """launch_clean_state_boxes: the positions of the cleaning operations of every launch"""
    out, done = [], 0
    while done < len(kinds):
        table = []
        while done < len(kinds) and len(table) < cap:
            if kinds[done] == "clean":
                table.append(done)
            done += 1
        if table:
            out.append(table)
    return out


def chunk_sizes(count, cap):
    """group_chunks: the chunks of `count` regions of one FAB"""
    out = [cap] * (count // cap)
    return out + ([count % cap] if count % cap else [])


def regions():
    """32 disjoint regions (lo, hi) of REGIONS_FAB, one inside every cell of REGIONS_CUTS: whole cells, cells trimmed on one side,
    and slabs one zone thick in x, y or z"""
    lo0 = REGIONS_FAB["lo"]
    cx, cy, cz = REGIONS_CUTS
    out = []
    for c in range(2):
        for b in range(4):
            for a in range(4):
                r = len(out)
                lo = [lo0[0] + cx[a], lo0[1] + cy[b], lo0[2] + cz[c]]
                hi = [lo0[0] + cx[a + 1] - 1, lo0[1] + cy[b + 1] - 1, lo0[2] + cz[c + 1] - 1]
                if r % 4 == 1:
                    lo[r % 3] += 1                              # trimmed
                elif r % 4 == 2:
                    hi[r % 3] = lo[r % 3]                       # one zone thick
                elif r % 4 == 3:
                    lo[(r + 1) % 3] = hi[(r + 1) % 3]
                out.append((tuple(lo), tuple(hi)))
    return out


def region_offsets(boxes, ncomp, empty=()):
    """offsets (in doubles) of the slices: handed out in the order r * 13 mod 32, not in region order, with a gap of 1 .. 5 doubles
    in front of every slice (an empty region takes a slice of no doubles) and a tail longer than any slice behind the last: a
    slice written at the offset of another region still ends inside the buffer.  (offsets, doubles of the buffer)"""
    n = len(boxes)
    tail = 1 + max(ncomp * zones(tuple(b[1][d] - b[0][d] + 1 for d in range(3))) for b in boxes)
    off, at = [0] * n, 0
    for q in range(n):
        r = (q * 13) % n if n == 32 else q
        at += 1 + r % 5
        off[r] = at
        if r not in empty:
            at += ncomp * zones(tuple(boxes[r][1][d] - boxes[r][0][d] + 1 for d in range(3)))
    return off, at + tail


def reduce_trips(ext, wg, max_wg):
    """launch_estdt / launch_clean_state_reduce: (zones a trip, trips, the k-plane each trip starts on or None)"""
    per = wg * max_wg
    n = zones(ext)
    plane = ext[0] * ext[1]
    starts = [t * per for t in range(ceil_div(n, per))]
    return per, len(starts), [s // plane if s % plane == 0 else None for s in starts]

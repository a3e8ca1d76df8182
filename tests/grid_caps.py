"""The shapes at which the tests cross the grid caps of the reduction and bottom-solve kernels, in one place (tests only): the GPU
tests import them, and tests/test_grid_caps_cpu.py reads the caps out of the kernel sources and asserts that every shape still
crosses its cap, and by how many trips -- a cap that is raised later fails that test instead of leaving the GPU tests below it.

The layout functions restate the launchers (launch_mg_norm, k_mg_bottom's loop, mp_layout, diag_layout, pack_layout) with the caps
as arguments; nothing here imports the product, torch or numpy."""

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

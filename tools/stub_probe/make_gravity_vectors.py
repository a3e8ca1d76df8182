#!/usr/bin/env python3
"""Generate tests/golden/stub_probe/gravity_vectors.npz: inputs and outputs of the reference's own Gravity::install_level,
compute_radial_mass, make_radial_gravity, interpolate_monopole_grav, add_pointmass_to_gravity, init_multipole_grav and
fill_multipole_BCs (Source/gravity/Gravity.cpp).

STUB-COMPILED, NOT a reference build (tools/stub_probe/README.md).  Gravity.cpp cannot be compiled in place: its other members pull
in MLMG, MLPoisson and FillPatchUtil.  So the seven member functions are compiled UNMODIFIED BUT NOT IN PLACE: slice() cuts the
verbatim text of each out of the reference's file at build time -- found by its signature line, taken to the matching closing
brace -- into one translation unit in a temporary directory, behind #include lines for the stand-ins (-DPROBE_GRAVITY) and for
the reference's own Gravity.H and Gravity_util.H, which are included unmodified and in place.  The recipe stops if a signature is
missing, occurs twice, or the braces do not balance.  That file is never kept: the committed artefacts are this recipe,
probe_gravity.cpp, the stand-ins and the vectors (data, written without time stamps: the same arrays give the same bytes).

Caveat of slicing: what the functions see of the rest of Gravity.cpp -- its includes, its file-scope variables, the constructor --
is the stand-ins' (probe_gravity.cpp), not the reference's.

The cases are described where they are made, and tools/stub_probe/README.md has the table.  The recipe stops if a case does not
hold the kind of zone it is there for."""
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CASTRO_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)
from make_vectors import read_blob, save_npz, write_blob   # noqa: E402

WANTED = ("install_level", "interpolate_monopole_grav", "compute_radial_mass", "make_radial_gravity", "add_pointmass_to_gravity",
          "init_multipole_grav", "fill_multipole_BCs")
NUM_GROW = 4


# ---- the slicing ---------------------------------------------------------------------------------------------------------------
def _closing_brace(text, at):
    """the index of the brace that closes the one at text[at], skipping comments, string and character literals"""
    depth, i, n = 0, at, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            i = text.index("\n", i)
        elif text.startswith("/*", i):
            i = text.index("*/", i) + 2
            continue
        elif c == '"' or c == "'":
            j = i + 1
            while text[j] != c:
                j += 2 if text[j] == "\\" else 1
            i = j
        elif c == "{":
            depth += 1
        elif c == "}":
            depth -= 1
            if depth == 0:
                return i
        i += 1
    raise SystemExit("slice: the braces do not balance")


def slice_functions(path, names):
    """the verbatim text of the member functions `names` of class Gravity in `path`, each from its return-type line to the
    closing brace of its body, in the order of `names`"""
    text = open(path).read()
    out = []
    for name in names:
        hits = [m for m in re.finditer(r"^Gravity::%s\s*\(" % re.escape(name), text, re.M)]
        if len(hits) != 1:
            raise SystemExit("slice: the signature of Gravity::%s occurs %d times in %s" % (name, len(hits), path))
        sig = hits[0].start()
        start = text.rfind("\n", 0, sig - 1) + 1                      # the line above holds the return type
        if text[start:sig].strip() != "void":
            raise SystemExit("slice: Gravity::%s does not follow a line that says `void`" % name)
        semi, brace = text.find(";", sig), text.find("{", sig)
        if brace < 0 or (0 <= semi < brace):
            raise SystemExit("slice: Gravity::%s has no body" % name)
        end = _closing_brace(text, brace)
        if text[end - 1] != "\n":
            raise SystemExit("slice: the body of Gravity::%s does not end at the start of a line" % name)
        body = text[start:end + 1]
        if re.search(r"^Gravity::", body[sig - start + 1:], re.M):
            raise SystemExit("slice: the body of Gravity::%s runs into the next function" % name)
        out.append(body)
    return out


def build(tmp):
    src = os.path.join(REF, "Source")
    subprocess.check_call([sys.executable, "set_variables.py", "--odir", tmp, "--nadv", "0", "--ngroups", "1", "--defines= ",
                           "_variables"], cwd=os.path.join(src, "driver"), stdout=subprocess.DEVNULL)
    tu = os.path.join(tmp, "gravity_sliced.cpp")
    with open(tu, "w") as f:
        f.write("#include <Castro_GravityProbe.H>\n#include <Gravity.H>\n#include <Gravity_util.H>\n\n")
        f.write("\n\n".join(slice_functions(os.path.join(src, "gravity", "Gravity.cpp"), WANTED)) + "\n")
    # the reference's Gravity.H must win over the stand-in of that name that probe_sources.cpp uses: its directory comes first
    flags = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DPROBE_GRAVITY", "-I" + os.path.join(src, "gravity"),
             "-I" + os.path.join(HERE, "stub"), "-I" + tmp]
    objs = []
    for path in (tu, os.path.join(HERE, "probe_gravity.cpp")):
        o = os.path.join(tmp, os.path.basename(path)[:-4] + ".o")
        subprocess.check_call(["g++"] + flags + ["-c", path, "-o", o])
        objs.append(o)
    exe = os.path.join(tmp, "probe_gravity")
    subprocess.check_call(["g++", "-o", exe] + objs)
    return exe


# ---- the cases -----------------------------------------------------------------------------------------------------------------
B1 = ((-3, 2, 1), (8, 8, 5))          # 12 x 7 x 5: crosses the 8 x 8 x 4 brick of the binning kernel in x and z
B2 = ((4, -2, -5), (6, 0, 3))         # 3 x 3 x 9
B3 = ((9, 2, 1), (10, 3, 2))          # 2 x 2 x 2, beside B1
DX_U, DX_D, DX_E = (0.05, 0.04, 0.0625), (0.125, 0.0625, 0.25), (0.125, 0.125, 0.125)
PROBLO = (-1.0, 0.5, 2.0)
NOWHERE = (-0.83, 0.71, 2.19)         # the middle of nothing; inside B1
DOM = ((0, 0, 0), (11, 6, 4))         # the 12 x 7 x 5 domain of the hierarchies and of the multipole cases
DOM8 = ((0, 0, 0), (7, 7, 7))


def shape(b):
    return tuple(b[1][d] - b[0][d] + 1 for d in (2, 1, 0))


def grow(b, ng):
    return tuple(x - ng for x in b[0]), tuple(x + ng for x in b[1])


def flat(boxes):
    return [float(x) for b in boxes for x in b[0] + b[1]]


def numpts(n):
    """Castro::get_numpts + 2 * NUM_GROW (Castro.cpp:2017-2024, :3887-3913) of a domain of n zones"""
    return int(math.sqrt(float(sum(x * x for x in n)))) + 2 * NUM_GROW


def full(rng, sh, lo=0.1, hi=10.0):
    return rng.uniform(lo, hi, size=sh)


def dyadic(rng, sh):
    """small multiples of powers of two: every sum of them, and of their products with a power of two, is exact in any order"""
    return rng.integers(1, 9, size=sh).astype(np.float64) * 2.0 ** rng.integers(-3, 4, size=sh)


def base(A, P, dx, center, boxes_by_level, domain=((0, 0, 0), (63, 63, 63)), drdxfac=1, is_flat=False, npts=None):
    n = tuple(domain[1][d] - domain[0][d] + 1 for d in range(3))
    A[P + "dx"], A[P + "problo"], A[P + "center"] = dx, PROBLO, center
    A[P + "probhi"] = [PROBLO[d] + n[d] * dx[d] for d in range(3)]
    A[P + "domain"] = flat([domain])
    A[P + "drdxfac"], A[P + "nlev"] = drdxfac, len(boxes_by_level)
    if is_flat:
        A[P + "flat"] = 1
    for l, bs in enumerate(boxes_by_level):
        A[P + "boxes%d" % l] = flat(bs)
        r = 1 if is_flat else 2 ** l
        A[P + "numpts%d" % l] = numpts([r * x for x in n]) if npts is None else npts[l]


def centres(b, dx, center, half=0.5):
    """problo + (index + half) dx - center of the zones of box b, broadcast to (nz, ny, nx)"""
    ax = [PROBLO[d] + (np.arange(b[0][d], b[1][d] + 1) + half) * dx[d] - center[d] for d in range(3)]
    return ax[0][None, None, :] + np.zeros(shape(b)), ax[1][None, :, None] + np.zeros(shape(b)), ax[2][:, None, None] + np.zeros(shape(b))


def zone_bin(b, dx, center, drdxfac):
    x, y, z = centres(b, dx, center)
    return np.floor(np.sqrt(x * x + y * y + z * z) * (1.0 / (dx[0] / float(drdxfac)))).astype(int)


def sub_bins(b, dx, center, f):
    """the bin of every sub-zone, (f^3, nz, ny, nx), with the operations of the function's own coordinates"""
    lo = centres(b, dx, center, 0.0)
    drinv = 1.0 / (dx[0] / float(f))
    out = []
    for kk in range(f):
        zz = lo[2] + (kk + 0.5) * (dx[2] / float(f))
        for jj in range(f):
            yy = lo[1] + (jj + 0.5) * (dx[1] / float(f))
            for ii in range(f):
                xx = lo[0] + (ii + 0.5) * (dx[0] / float(f))
                out.append(np.sqrt(xx * xx + yy * yy + zz * zz) * drinv)
    return np.array(out)


def stop_unless(ok, what):
    if not ok:
        raise SystemExit("make_gravity_vectors: " + what)


def radial_mass_cases(rng, A):
    """rm<c>: compute_radial_mass.  Two families: uneven dx with full-mantissa densities (the order of the sums is the loop
    nest's), dyadic dx with densities that are small multiples of powers of two (every sum exact in any order)"""
    on_lo = tuple(PROBLO)
    cases = [
        # dx, centre, boxes, drdxfac, n1d (None: the natural one), density
        (DX_U, NOWHERE, [B1, B2], 1, None, full),
        (DX_U, NOWHERE, [B1], 2, None, full),
        (DX_U, NOWHERE, [B1, B2, B3], 4, None, full),
        (DX_U, NOWHERE, [B1, B2], 2, "short", full),
        (DX_U, NOWHERE, [B1], 2, None, "zeros"),
        (DX_U, on_lo, [B1, B2], 1, None, full),                                               # octant factor 8
        (DX_U, tuple(PROBLO[d] + 0.009 * DX_U[d] for d in range(3)), [B1, B2], 2, None, full),   # still 8
        (DX_U, (PROBLO[0] + 0.011 * DX_U[0], PROBLO[1], PROBLO[2]), [B1, B2], 2, None, full),    # 1
        (DX_D, NOWHERE, [B1, B2], 2, None, dyadic),
        (DX_D, NOWHERE, [B1, B2, B3], 4, "short", dyadic),
        # a sub-zone radius that is an exact multiple of dr.  With the centre on a zone corner no such sub-zone exists for any
        # dyadic dx: x / dr is then half an odd number, and p^2 + 4^a q^2 + 4^b s^2 = 4 n^2 has no solution with p odd.  So the
        # centre is the middle of a zone (drdxfac 1) or of a sub-zone (drdxfac 2), and the 3-4-5 sub-zone lies in its plane
        (DX_E, tuple(PROBLO[d] + (i + 0.5) * DX_E[d] for d, i in enumerate((1, 4, 3))), [B1], 1, None, dyadic),
        (DX_E, tuple(PROBLO[d] + (i + 0.25) * DX_E[d] for d, i in enumerate((1, 4, 3))), [B1, B2], 2, None, dyadic),
        (DX_D, on_lo, [B1, B2], 2, None, "dzeros"),
    ]
    for c, (dx, center, boxes, f, n1d, dens) in enumerate(cases):
        P = "rm%d." % c
        base(A, P, dx, center, [boxes, boxes], drdxfac=f, is_flat=True)
        bins = np.concatenate([zone_bin(b, dx, center, f).ravel() for b in boxes])
        if n1d is None:
            A[P + "level"], A[P + "n1d"] = 0, f * A[P + "numpts0"]
            stop_unless(bins.max() < A[P + "n1d"], P + "level 0 aborts beyond the last bin")
        else:
            A[P + "level"], A[P + "n1d"] = 1, int(np.median(bins))
        for b, bx in enumerate(boxes):
            if dens in ("zeros", "dzeros"):
                rho = (dyadic if dens == "dzeros" else full)(rng, shape(bx))
                hole = rng.uniform(size=shape(bx)) < 0.2
                rho[hole] = 0.0
                rho[1, 2, 2], rho[2, 0, 1] = -0.0, -0.0
                stop_unless(hole.sum() > 3 and np.signbit(rho[rho == 0.0]).sum() >= 2, P + "zeros of both signs")
            else:
                rho = dens(rng, shape(bx))
            A[P + "rho0_%d" % b] = A[P + "rho1_%d" % b] = rho
        if n1d == "short":
            n, zb = A[P + "n1d"], bins
            sb = np.concatenate([np.floor(sub_bins(b, dx, center, f)).reshape(f ** 3, -1) for b in boxes], axis=1)
            stop_unless(((zb > n - 1) & (sb <= n - 1).any(axis=0)).any(), P + "a dropped zone with sub-zones inside")
            stop_unless(((zb <= n - 1) & (sb > n - 1).any(axis=0)).any(), P + "a kept zone with sub-zones beyond")
            stop_unless((zb <= n - 1).any() and (zb > n - 1).any(), P + "zones on both sides of the last bin")
        if dx is DX_E:
            sb = np.concatenate([sub_bins(b, dx, center, f).ravel() for b in boxes])
            stop_unless(((sb == np.floor(sb)) & (sb > 0)).any() and (sb == 5.0).any(), P + "a sub-zone on a bin edge")


# the hierarchies of rg<c> and mp<c>: level 1 over the coarse zones (2..5, 1..4, 1..3), level 2 over the level-1 zones (6..9, 4..7, 3..5)
L1 = ((4, 2, 2), (11, 9, 7))
L1A, L1B = ((4, 2, 2), (7, 9, 7)), ((8, 2, 2), (11, 9, 7))
L2 = ((12, 8, 6), (19, 15, 11))


def fine_mask(crse_boxes, fine_boxes):
    """Castro::build_fine_mask: 1, and 0 where a box of the level above covers the zone"""
    out = []
    for cb in crse_boxes:
        m = np.ones(shape(cb))
        for fb in fine_boxes:
            lo = [fb[0][d] // 2 for d in range(3)]
            hi = [fb[1][d] // 2 for d in range(3)]
            sl = tuple(slice(max(lo[d], cb[0][d]) - cb[0][d], min(hi[d], cb[1][d]) - cb[0][d] + 1) for d in (2, 1, 0))
            m[sl] = 0.0
        out.append(m)
    return out


def radial_gravity_cases(rng, A):
    """rg<c>: install_level + make_radial_gravity on hierarchies of one, two and three levels"""
    mid = (-0.7, 0.64, 2.16)                       # probhi - centre = (0.3, 0.14, 0.1525): max_radius_all_in_domain = 0.14
    probhi_u = [PROBLO[d] + (DOM[1][d] + 1) * DX_U[d] for d in range(3)]
    DX_Q = (0.0625, 0.0625, 0.0625)
    cases = [
        # dx, centre, levels, argument level, drdxfac, (t_old, t_new) per level, time, density, what
        (DX_U, mid, [[DOM]], 0, 1, [(0.0, 1.0)], 0.0, full, None),                           # time == t_old; maxrad mid-array
        (DX_U, (-0.7, probhi_u[1] - 0.03, 2.16), [[DOM]], 0, 2, [(0.0, 1.0)], 1.0, full, None),   # t_new; maxrad below the centre of bin 1
        (DX_U, (-0.75, 0.6, 2.15), [[DOM]], 0, 1, [(0.25, 0.75)], 0.4, full, "empty"),       # in between; bin 2 empty, the last below maxrad
        (DX_Q, (-0.625, 0.78125, 2.15625), [[DOM]], 0, 1, [(0.5, 0.5)], 0.5, dyadic, "rc"),  # eps == 0; rc of bin 2 == maxrad
        (DX_U, mid, [[DOM]], 0, 2, [(0.0, 1.0)], 1.0, full, "short"),                        # maxrad beyond the last bin
        (DX_U, mid, [[DOM], [L1]], 1, 2, [(0.0, 1.0), (0.0, 0.5)], 0.3, full, None),         # both levels in between
        ((0.0625, 0.03125, 0.125), mid, [[DOM], [L1A, L1B]], 1, 1, [(0.0, 1.0), (0.5, 1.0)], 1.0, dyadic, None),
        (DX_U, mid, [[DOM], [L1], [L2]], 2, 1, [(0.0, 1.0), (0.0, 0.5), (0.25, 0.5)], 0.3, full, None),
    ]
    for c, (dx, center, levels, level, f, times, time, dens, what) in enumerate(cases):
        P = "rg%d." % c
        npts = [2] if what == "short" else None
        base(A, P, dx, center, levels, domain=DOM, drdxfac=f, npts=npts)
        A[P + "level"], A[P + "time"] = level, time
        maxrad = min(A[P + "probhi"][d] - center[d] for d in range(3))
        dr = dx[0] / float(f)
        for l, bs in enumerate(levels):
            A[P + "t_old%d" % l], A[P + "t_new%d" % l] = times[l]
            dxl = tuple(x / 2 ** l for x in dx)
            for b, bx in enumerate(bs):
                old, new = dens(rng, shape(bx)), dens(rng, shape(bx))
                zb = zone_bin(bx, dxl, center, f)
                if what == "empty":
                    old[zb == 2], new[zb == 2] = 0.0, 0.0
                    stop_unless((zb == 2).any() and 2.5 * dr < maxrad < 3.5 * dr, P + "bin 2 is the last below maxrad")
                if what == "short":
                    n1d = f * npts[0]
                    old[zb > n1d - 1], new[zb > n1d - 1] = 0.0, 0.0
                    stop_unless(maxrad > n1d * dr and (zb <= n1d - 1).any(), P + "maxrad beyond the last bin")
                A[P + "rho_old%d_%d" % (l, b)], A[P + "rho_new%d_%d" % (l, b)] = old, new
            if l + 1 < len(levels):
                for b, m in enumerate(fine_mask(bs, levels[l + 1])):
                    A[P + "mask%d_%d" % (l, b)] = m
                    stop_unless((m == 0.0).any() and (m == 1.0).any(), P + "masked and unmasked zones")
        if what == "rc":
            stop_unless(maxrad == 2.5 * dr, P + "rc of bin 2 equals maxrad to the bit")
        if c == 1:
            stop_unless(maxrad < 1.5 * dr, P + "maxrad below the centre of bin 1")
        if c == 0:
            stop_unless(1.5 * dr < maxrad < (f * A[P + "numpts0"] - 1) * dr, P + "maxrad mid-array")


def interpolate_cases(rng, A):
    """ig<c>: interpolate_monopole_grav onto FABs grown by two zones that hold a sentinel, called with level 1 (level 0 aborts
    beyond the last bin)"""
    zc = tuple(PROBLO[d] + (i + 0.5) * DX_U[d] for d, i in enumerate((3, 5, 3)))
    cases = [
        (NOWHERE, 1, [-1.0, -3.0, -2.5, -6.0, -1.5, -4.0, -2.0]),
        (tuple(zc[d] + 0.1 * DX_U[d] for d in range(3)), 2, [-0.3, -2.2, -2.4, -5.1, -5.0, -1.2, -1.1, -3.9, -0.8, -4.4, -4.6, -2.0, -6.3]),
        (tuple(zc[d] + 1.0e-3 * DX_U[d] for d in range(3)), 1, [-2.0, -1.0, -4.0, -3.5, -7.0, -0.5, -0.75, -5.0]),
    ]
    for c, (center, f, prof) in enumerate(cases):
        P = "ig%d." % c
        base(A, P, DX_U, center, [[B1, B2], [B1, B2]], drdxfac=f, is_flat=True)
        A[P + "level"], A[P + "ng"], A[P + "fill"] = 1, 2, 7.25e33
        A[P + "rg"] = np.array(prof) * rng.uniform(0.9, 1.1, size=len(prof))
        n1d = len(prof)
        zb = zone_bin(grow(B1, 2), DX_U, center, f)
        stop_unless((zb == 0).any() and (zb == n1d - 1).any() and (zb > n1d - 1).any() and ((zb > 0) & (zb < n1d - 1)).any(),
                    P + "zones in bin 0, in the last bin, in between and beyond")


def pointmass_cases(rng, A):
    """pg<c>: add_pointmass_to_gravity; grav has more ghost zones than phi"""
    corner = tuple(PROBLO[d] + i * DX_U[d] for d, i in enumerate((2, 5, 3)))
    cases = [(corner, 2.0e33, [B1, B2], 2, 1), (NOWHERE, 0.02, [B1, B2], 2, 1), (NOWHERE, 1.0e30, [B1], 1, 0)]
    for c, (center, mass, boxes, ngg, ngp) in enumerate(cases):
        P = "pg%d." % c
        base(A, P, DX_U, center, [boxes])
        A[P + "mass"], A[P + "ng_grav"], A[P + "ng_phi"] = mass, ngg, ngp
        for b, bx in enumerate(boxes):
            for n in range(3):
                A[P + "grav%d_%d" % (n, b)] = rng.uniform(-1.0, 1.0, size=shape(grow(bx, ngg))) * 1.0e3
            A[P + "phi%d" % b] = rng.uniform(-1.0, 1.0, size=shape(grow(bx, ngp))) * 1.0e5


def multipole_cases(rng, A):
    """mp<c>: init_multipole_grav + fill_multipole_BCs, outflow on every face (no Symmetry face)"""
    def mid(dom, dx):
        return tuple(PROBLO[d] + 0.5 * (dom[1][d] + 1) * dx[d] for d in range(3))
    DX_Q = (0.0625, 0.0625, 0.0625)
    L1_8 = ((4, 4, 2), (11, 11, 9))
    cases = [
        (DOM, DX_U, mid(DOM, DX_U), 0, [[DOM]]),
        (DOM, DX_U, (-0.83, 0.71, 2.19), 2, [[DOM]]),
        (DOM, DX_U, mid(DOM, DX_U), 6, [[DOM], [L1]]),
        (DOM8, DX_Q, tuple(PROBLO), 2, [[DOM8]]),                   # the corner ghost zone (-1, -1, -1) has r = 0
        (DOM8, DX_Q, (-0.8, 0.81, 2.2), 6, [[DOM8], [L1_8]]),
        (DOM, DX_U, tuple(PROBLO), 6, [[DOM]]),
    ]
    for c, (dom, dx, center, lnum, levels) in enumerate(cases):
        P = "mp%d." % c
        base(A, P, dx, center, levels, domain=dom)
        A[P + "lnum"] = lnum
        for l, bs in enumerate(levels):
            for b, bx in enumerate(bs):
                A[P + "rho%d_%d" % (l, b)] = full(rng, shape(bx)) * 10.0 ** rng.integers(0, 3)
            if l + 1 < len(levels):
                for b, m in enumerate(fine_mask(bs, levels[l + 1])):
                    A[P + "mask%d_%d" % (l, b)] = m
        A[P + "phi0"] = rng.uniform(-1.0, 1.0, size=shape(grow(dom, 1))) * 1.0e-6
        x, y, z = centres(dom, dx, center)
        stop_unless((np.sqrt(x * x + y * y + z * z) > 0.0).all(), P + "no zone is centred on the centre (NaN moments)")


def main():
    rng = np.random.default_rng(20261021)
    A = {}
    radial_mass_cases(rng, A)
    radial_gravity_cases(rng, A)
    interpolate_cases(rng, A)
    pointmass_cases(rng, A)
    multipole_cases(rng, A)
    A = {k: np.asarray(v, dtype=np.float64) for k, v in A.items()}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        write_blob(os.path.join(tmp, "in.bin"), A)
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
        O = read_blob(os.path.join(tmp, "out.bin"))
    allv = {"in:" + k: np.atleast_1d(v) for k, v in A.items()}
    for k, v in O.items():
        P, name = k.split(".")
        if name.startswith("grav") and not P.startswith("rg"):
            b = int(name[4:])
            bx = [B1, B2][b] if P.startswith("ig") else _boxes(A, P, 0)[b]
            v = v.reshape((3,) + shape(grow(bx, int(A[P + (".ng" if P.startswith("ig") else ".ng_grav")]))))
        elif name.startswith("phi"):
            v = v.reshape(A[P + "." + name].shape)
        allv["out:" + k] = v
    # what the cases are there for and only the outputs can show
    for c in range(64):
        P = "ig%d." % c
        if "in:" + P + "fill" in allv:
            g = allv["out:" + P + "grav0"]
            stop_unless((g == A[P + "fill"]).any() and (g != A[P + "fill"]).any(),
                        P + "zones beyond the last bin keep the sentinel")
        P = "mp%d." % c
        if "in:" + P + "lnum" in allv:
            phi, was = allv["out:" + P + "phi0"], A[P + "phi0"]
            stop_unless(np.array_equal(phi[1:-1, 1:-1, 1:-1], was[1:-1, 1:-1, 1:-1]), P + "the interior of phi is untouched")
            stop_unless((phi[0, 0, 0] == 0.0) == (tuple(A[P + "center"]) == PROBLO), P + "the r < 1e-12 zone")
    dst = os.path.join(ROOT, "tests", "golden", "stub_probe", "gravity_vectors.npz")
    save_npz(dst, allv)
    print("wrote %s: %d input arrays, %d output arrays, %.1f KB" % (dst, len(A), len(O), os.path.getsize(dst) / 1024.0))


def _boxes(A, P, l):
    a = [int(x) for x in A[P + ".boxes%d" % l]]
    return [(tuple(a[i:i + 3]), tuple(a[i + 3:i + 6])) for i in range(0, len(a), 6)]


if __name__ == "__main__":
    main()

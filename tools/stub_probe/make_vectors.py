#!/usr/bin/env python3
"""Generate tests/golden/stub_probe/vectors.npz: inputs and outputs of the reference's own per-zone functions.

STUB-COMPILED, NOT oracle/_ref.  The reference cannot be built in this image (AMReX and Microphysics are empty
submodules, Exec/Make.Castro:24-26,44-46), so this script compiles the reference's hydro sources UNMODIFIED and IN PLACE
from /root/reference against the stand-in headers in tools/stub_probe/stub/ (about 250 lines: Array4, Box, ParallelFor,
Geometry, a gamma-law eos(), the castro:: parameters) and runs probe.cpp on seeded inputs.  state_indices.H is produced
by the reference's own Source/driver/set_variables.py into a temporary directory.  What this shows: whether the
oracle's C restatement and the device functions of ppm_reconstruct / ppm_int_profile, uflatten, cmpflx_plus_godunov
(CGF, CG with every cg_blend, HLLC, HLL), actual_trans_single / actual_trans_final, ctoprim and trace_ppm have slipped
from the source text they follow.  What it does NOT show: anything about a real reference binary (AMReX's Array4 /
ParallelFor, Microphysics's EOS arithmetic order) -- parity stays "unpinned" (DESIGN.md section 6).

Only runs where /root/reference exists; nothing of the reference's sources is copied into the repository: the committed
artefacts are this recipe and the vectors (data)."""
import io
import os
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CASTRO_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
from tests.util import physical_state   # noqa: E402


def write_blob(path, arrays):
    with open(path, "wb") as f:
        for name, a in arrays.items():
            a = np.ascontiguousarray(np.atleast_1d(np.asarray(a, dtype=np.float64))).ravel()
            f.write(name.encode().ljust(48, b"\0"))
            f.write(struct.pack("<q", a.size))
            f.write(a.tobytes())


def read_blob(path):
    out = {}
    with open(path, "rb") as f:
        while True:
            h = f.read(48)
            if len(h) < 48:
                break
            n = struct.unpack("<q", f.read(8))[0]
            out[h.split(b"\0")[0].decode()] = np.frombuffer(f.read(8 * n), dtype=np.float64).copy()
    return out


def build(tmp):
    src = os.path.join(REF, "Source")
    subprocess.check_call([sys.executable, "set_variables.py", "--odir", tmp, "--nadv", "0", "--ngroups", "1", "--defines= ",
                           "_variables"], cwd=os.path.join(src, "driver"), stdout=subprocess.DEVNULL)
    inc = ["-I" + os.path.join(HERE, "stub"), "-I" + tmp, "-I" + os.path.join(src, "hydro"), "-I" + os.path.join(src, "driver"),
           "-I" + os.path.join(src, "problems"), "-I" + os.path.join(src, "rotation")]
    flags = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math"]
    objs = []
    for f in ("trans", "flatten", "riemann", "riemann_util", "advection_util", "trace_ppm", "trace_plm", "Castro_ctu", "edge_util"):
        o = os.path.join(tmp, f + ".o")
        subprocess.check_call(["g++"] + flags + inc + ["-c", os.path.join(src, "hydro", f + ".cpp"), "-o", o])
        objs.append(o)
    for f in ("probe", "probe_params"):
        o = os.path.join(tmp, f + ".o")
        subprocess.check_call(["g++"] + flags + inc + ["-c", os.path.join(HERE, f + ".cpp"), "-o", o])
        objs.append(o)
    exe = os.path.join(tmp, "probe")
    subprocess.check_call(["g++", "-o", exe] + objs)
    # the problem initialisers (Exec/hydro_tests/{Sedov,Sod}) in their own executable
    o = os.path.join(tmp, "probe_init.o")
    subprocess.check_call(["g++"] + flags + inc + ["-DREFERENCE_EXEC=" + os.path.join(REF, "Exec", "hydro_tests"), "-c",
                                                   os.path.join(HERE, "probe_init.cpp"), "-o", o])
    subprocess.check_call(["g++", "-o", exe + "_init", o, os.path.join(tmp, "probe_params.o")])
    # the derived fields (Source/driver/Derive.cpp, unmodified)
    od = [os.path.join(tmp, "Derive.o"), os.path.join(tmp, "probe_derive.o"), os.path.join(tmp, "timestep.o")]
    subprocess.check_call(["g++"] + flags + inc + ["-c", os.path.join(src, "driver", "Derive.cpp"), "-o", od[0]])
    subprocess.check_call(["g++"] + flags + inc + ["-c", os.path.join(src, "driver", "timestep.cpp"), "-o", od[2]])
    subprocess.check_call(["g++"] + flags + inc + ["-c", os.path.join(HERE, "probe_derive.cpp"), "-o", od[1]])
    subprocess.check_call(["g++", "-o", exe + "_derive"] + od + [os.path.join(tmp, "probe_params.o")])
    # the rotation sources (Source/rotation/rotation_sources.cpp, Rotation.cpp, unmodified)
    orot = []
    for path in (os.path.join(src, "rotation", "rotation_sources.cpp"), os.path.join(src, "rotation", "Rotation.cpp"),
                 os.path.join(HERE, "probe_rotation.cpp")):
        o = os.path.join(tmp, "rot_" + os.path.basename(path)[:-4] + ".o")
        subprocess.check_call(["g++"] + flags + inc + ["-c", path, "-o", o])
        orot.append(o)
    subprocess.check_call(["g++", "-o", exe + "_rotation"] + orot + [os.path.join(tmp, "probe_params.o")])
    # the source terms added since (Castro_sponge.cpp, Castro_gravity.cpp, Castro_pointmass.cpp, unmodified); the stand-in Castro
    # grows by what they touch only under PROBE_SOURCES, so the executables above see the class they always saw
    osrc = []
    for path in (os.path.join(src, "sources", "Castro_sponge.cpp"), os.path.join(src, "gravity", "Castro_gravity.cpp"),
                 os.path.join(src, "gravity", "Castro_pointmass.cpp"), os.path.join(HERE, "probe_sources.cpp"),
                 os.path.join(HERE, "probe_params.cpp")):
        o = os.path.join(tmp, "src_" + os.path.basename(path)[:-4] + ".o")
        subprocess.check_call(["g++"] + flags + inc + ["-DPROBE_SOURCES", "-DSPONGE", "-DGRAVITY", "-I" + os.path.join(src, "sources"),
                                                       "-I" + os.path.join(src, "gravity"), "-c", path, "-o", o])
        osrc.append(o)
    subprocess.check_call(["g++", "-o", exe + "_sources"] + osrc)
    # the boundary overrides of the state fill (Source/problems/ambient_fill.cpp, hse_fill.cpp, unmodified); the stand-ins grow by
    # what they touch only under PROBE_BC
    obc = []
    for path in (os.path.join(src, "problems", "ambient_fill.cpp"), os.path.join(src, "problems", "hse_fill.cpp"),
                 os.path.join(HERE, "probe_bc.cpp"), os.path.join(HERE, "probe_params.cpp")):
        o = os.path.join(tmp, "bc_" + os.path.basename(path)[:-4] + ".o")
        subprocess.check_call(["g++"] + flags + inc + ["-DPROBE_BC", "-DGRAVITY", "-c", path, "-o", o])
        obc.append(o)
    subprocess.check_call(["g++", "-o", exe + "_bc"] + obc)
    o = os.path.join(tmp, "bc_hse_fill_silent.o")
    subprocess.check_call(["g++"] + flags + inc + ["-DPROBE_BC", "-DGRAVITY", "-DAMREX_USE_GPU", "-c",
                                                   os.path.join(src, "problems", "hse_fill.cpp"), "-o", o])
    subprocess.check_call(["g++", "-o", exe + "_bc_silent"] + [o if x.endswith("bc_hse_fill.o") else x for x in obc])
    return exe


# ---- the source terms: sponge<c>.*, grav<c>.*, pm<c>.* of tests/golden/stub_probe/source_vectors.npz ---------------------------
K_B, M_U, GAMMA = 1.3806488e-16, 1.660538921e-24, 1.4          # stub/eos.H
SRC_DX, SRC_PROBLO = (0.05, 0.04, 0.0625), (-1.0, 0.5, 2.0)
# two small awkward boxes: 12 x 7 x 5 with a negative low x index, 3 x 3 x 9 with negative low y and z indices.  row: the axis
# and the zone (the other two indices) of the line of zones the centre is put on, so that |r| is exact there; on: the two
# indices along that axis whose zones sit exactly on the lower and the upper radius; free: the centre's coordinate along the row
SRC_BOXES = [dict(lo=(-3, 2, 1), hi=(8, 8, 5), row=0, at=(None, 4, 3), on=(4, 7), free=-0.9137),
             dict(lo=(4, -2, -5), hi=(6, 0, 3), row=2, at=(5, -1, None), on=(0, 2), free=1.9291)]
SPONGE_RAMPS = dict(radius=("lower_radius", "upper_radius"), density=("lower_density", "upper_density"),
                    step=("lower_density", "upper_density"), pressure=("lower_pressure", "upper_pressure"))
# (ramps, implicit, target velocity, timescale): tests/test_sponge_gpu.py::ZONE_CASES, then two ramps at once and alpha = 0
SPONGE_CASES = [((w,), imp, (0.0, 0.0, 0.0), 2.e-3) for w in ("radius", "step", "pressure") for imp in (1, 0)] \
    + [(("radius", "density", "pressure"), imp, (0.0, 0.0, 0.0), 2.e-3) for imp in (1, 0)] \
    + [(("radius", "density", "pressure"), 1, (0.4, -0.3, 0.2), 2.e-3), (("density",), 0, (-0.1, 0.2, 0.3), 2.e-3),
       (("density",), 1, (0.0, 0.0, 0.0), 2.e-3), (("radius", "density"), 1, (0.4, -0.3, 0.2), 2.e-3),
       (("radius", "pressure"), 0, (0.0, 0.0, 0.0), 2.e-3), (("density",), 1, (0.0, 0.1, 0.0), -1.0), (("radius",), 0, (0.0, 0.0, 0.0), 0.0)]


def _shape(lo, hi, grow=0):
    return tuple(hi[a] - lo[a] + 1 + 2 * grow for a in (2, 1, 0))


def _coarse(rng, shape):
    """positive values of a few bits each, for the components a function does not read or only copies: they differ from zone
    to zone and from every component it does read, and cost the fixture a quarter of a full mantissa"""
    return rng.integers(1, 4096, size=shape) / 64.0


def _pressure(rho, T, rhoX):
    """eos(eos_input_rt) of stub/eos.H with one species of A = 1, as Castro_sponge.cpp:161-176 calls it"""
    xn = rhoX * (1.0 / rho)
    mu = 1.0 / (0.0 + xn * 1.0)
    e = K_B * T / ((GAMMA - 1.0) * (mu * M_U))
    return (GAMMA - 1.0) * rho * e


def sponge_inputs(rng, A):
    for c, (ramps, implicit, vt, timescale) in enumerate(SPONGE_CASES):
        P, b = "sponge%d." % c, SRC_BOXES[0 if c % 3 == 0 else 1]          # the larger box for every third case: the fixture's size
        lo, hi, shp = b["lo"], b["hi"], _shape(b["lo"], b["hi"])
        n = int(np.prod(shp))
        rho = 10.0 ** rng.uniform(-1.0, 1.0, n)
        T = 10.0 ** rng.uniform(-9.0, -7.0, n)                       # p / rho between 0.08 and 8
        X = rho * rng.uniform(0.9, 1.0, n)
        vel = rng.normal(size=(3, n))
        vel[:, 5:8] = 0.0                                            # three zones at rest
        par = dict(lower_radius=-1.0, upper_radius=-1.0, lower_density=-1.0, upper_density=-1.0, lower_pressure=-1.0,
                   upper_pressure=-1.0)
        # the centre: on the line of zone centres b["row"], at b["free"] along it -- not the middle of anything
        zc = lambda d, i: SRC_PROBLO[d] + (float(i) + 0.5) * SRC_DX[d]
        center = [b["free"] if d == b["row"] else zc(d, b["at"][d]) for d in range(3)]
        if "radius" in ramps:
            r = [zc(b["row"], i) - center[b["row"]] for i in b["on"]]
            par["lower_radius"], par["upper_radius"] = [float(np.sqrt(x * x + 0.0 * 0.0 + 0.0 * 0.0)) for x in r]
        if "density" in ramps:
            par["lower_density"], par["upper_density"] = 0.5, 2.0
            rho[1], rho[2] = 0.5, 2.0                                # exactly on the two cutoffs
            X[1:3] = rho[1:3] * 0.95
        if "step" in ramps:                                          # lower == upper: no zone on it (0 / 0 in the ramp)
            par["lower_density"], par["upper_density"] = 1.0, 1.0
        if "pressure" in ramps:
            rho[3], T[3], rho[4], T[4] = 1.5, 2.4e-8, 0.6, 6.1e-9    # p close to 3 and to 0.3: these two zones ARE the cutoffs
            X[3:5] = rho[3:5] * 0.97
            par["upper_pressure"], par["lower_pressure"] = float(_pressure(rho[3], T[3], X[3])), float(_pressure(rho[4], T[4], X[4]))
        U = np.zeros((8, n))
        U[0], U[6], U[7] = rho, T, X
        for k in range(3):
            U[1 + k] = rho * vel[k]
        U[4], U[5] = _coarse(rng, n), _coarse(rng, n)                 # apply_sponge reads neither energy
        A[P + "box"], A[P + "dx"], A[P + "problo"], A[P + "center"] = np.array(lo + hi, dtype=np.float64), SRC_DX, SRC_PROBLO, center
        A[P + "U"], A[P + "dt"], A[P + "eos_gamma"] = U.reshape((8,) + shp), 3.7e-3, GAMMA
        # with these two, lower_factor + 0.5 (upper_factor - lower_factor) (1 - cos(pi)) is one ulp above upper_factor: the zone
        # on the far cutoff of a ramp tells the reference's inclusive comparison from an exclusive one
        A[P + "lower_factor"], A[P + "upper_factor"] = 0.07, 0.874
        A[P + "target_velocity"], A[P + "timescale"], A[P + "implicit"] = vt, timescale, float(implicit)
        for k, v in par.items():
            A[P + k] = v


def gravity_inputs(rng, A):
    for c in range(8):
        P, b = "grav%d." % c, SRC_BOXES[0 if c in (3, 4, 7) else 1]
        lo, hi, shp = b["lo"], b["hi"], _shape(b["lo"], b["hi"])
        n = int(np.prod(shp))
        uold, unew = _coarse(rng, (8, n)), _coarse(rng, (8, n))              # the sources read the density and the momenta only
        uold[0] = 10.0 ** rng.uniform(-1.0, 1.0, n)
        unew[0] = uold[0] * rng.choice([1.0, 1.1, 0.9, 10.0, 0.1], n)       # the density changes by up to a factor of ten
        for U in (uold, unew):
            U[1:4] = U[0] * rng.normal(size=(3, n)) * 10.0 ** rng.uniform(-1.0, 1.0, n)
        uold[1:4, 4:7] = 0.0                                                # at rest at the old time, at both times, at the new time
        unew[1:4, 5:8] = 0.0
        A[P + "box"], A[P + "dx"], A[P + "problo"], A[P + "center"] = np.array(lo + hi, dtype=np.float64), SRC_DX, SRC_PROBLO, (0.1, 0.9, 2.1)
        A[P + "uold"], A[P + "unew"] = uold.reshape((8,) + shp), unew.reshape((8,) + shp)
        gshp = (3,) + _shape(lo, hi, 1)
        if c < 4:                                                           # one vector in every zone, ghost zones included
            g = np.empty(gshp)
            for k, v in enumerate((0.3, -0.7, -9.8)):
                g[k] = v
            A[P + "gold"], A[P + "gnew"] = g, g.copy()
        else:
            A[P + "gold"], A[P + "gnew"] = rng.normal(size=gshp), rng.normal(size=gshp)
        for d in range(3):
            fhi = list(hi)
            fhi[d] += 1
            A[P + "mflux%d" % d] = rng.normal(scale=1e-3, size=_shape(lo, fhi))
        A[P + "grav_source_type"], A[P + "dt"], A[P + "const"] = float(1 + c % 4), 0.013, float(c < 4)


# (boxes, icen, centre at a zone corner, kind).  kind "+", "-", "0": full-mantissa densities, one box -- the order of the
# reference's sum is then the loop nest's.  "d+", "d-", "d0", "d-+": several boxes, dx and every density a small multiple of a
# power of two, so that vol * (rho_new - rho_old) and every partial sum are exact: across boxes (ranks, threads) the reference
# fixes no order, and the recorded total is the same in any.  "d0": the parts cancel to exactly zero.  "d-+": the first box's
# part is negative, the total positive.
_A, _B = SRC_BOXES[0], SRC_BOXES[1]
PM_CASES = [([(_A["lo"], _A["hi"])], (3, 5, 3), False, "+"),
            ([(_A["lo"], _A["hi"])], (3, 5, 3), True, "-"),
            ([(_A["lo"], _A["hi"])], (4, 6, 2), False, "0"),
            ([((-3, 2, 1), (2, 8, 5)), ((3, 2, 1), (8, 8, 5))], (3, 5, 3), True, "d+"),
            ([((-3, 2, 1), (8, 4, 5)), ((-3, 5, 1), (8, 8, 5))], (3, 5, 3), False, "d-"),
            ([(_B["lo"], _B["hi"])], (5, -1, 0), False, "+"),                  # the cube sticks out of the box in x and y
            ([((4, -2, -5), (6, 0, -2)), ((4, -2, -1), (6, 0, 0)), ((4, -2, 1), (6, 0, 3))], (5, -1, 0), True, "d0"),
            ([((-3, 2, 1), (2, 8, 5)), ((3, 2, 1), (8, 8, 5))], (3, 5, 3), False, "d-+"),
            ([(_B["lo"], _B["hi"])], (5, -1, 0), True, "-"),
            # four slabs in x of which the first and the last miss the cube (x = 1 .. 4): their parts are 0, their S_new stays
            ([((-3, 2, 1), (-1, 8, 5)), ((0, 2, 1), (2, 8, 5)), ((3, 2, 1), (5, 8, 5)), ((6, 2, 1), (8, 8, 5))], (3, 5, 3), False, "d+"),
            # the cube cut in all three directions at once: eight boxes, an eighth of the cube in each
            ([((x0, y0, z0), (x1, y1, z1)) for (z0, z1) in ((1, 2), (3, 5)) for (y0, y1) in ((2, 4), (5, 8)) for (x0, x1) in ((-3, 2), (3, 8))],
             (3, 5, 3), True, "d+")]


def pointmass_inputs(rng, A):
    for c, (boxes, icen, corner, kind) in enumerate(PM_CASES):
        P = "pm%d." % c
        dyadic = kind.startswith("d")
        dx, problo = ((0.125, 0.25, 0.0625), (-0.5, 1.0, 0.25)) if dyadic else ((0.1, 0.12, 0.15), (-0.3, 0.0, 0.2))
        frac = (0.0, 0.0, 0.0) if corner else (0.3, 0.6, 0.45)
        center = [problo[d] + (icen[d] + frac[d]) * dx[d] for d in range(3)]
        clo, chi = [i - 2 for i in icen], [i + 1 for i in icen]
        A[P + "boxes"] = np.array([x for lo, hi in boxes for x in lo + hi], dtype=np.float64)
        A[P + "dx"], A[P + "problo"], A[P + "center"], A[P + "mass"] = dx, problo, center, 3.0e9 if not dyadic else 4096.0
        olds, news, cubes = [], [], []
        for b, (lo, hi) in enumerate(boxes):
            shp = _shape(lo, hi)
            if dyadic:
                so, sn = rng.integers(32, 129, size=(8,) + shp) / 64.0, rng.integers(32, 129, size=(8,) + shp) / 64.0
            else:
                so, sn = _coarse(rng, (8,) + shp), _coarse(rng, (8,) + shp)     # the restore copies every component
                so[0], sn[0] = rng.uniform(0.5, 2.0, size=shp), rng.uniform(0.5, 2.0, size=shp)
            cut = [(max(clo[d], lo[d]), min(chi[d], hi[d])) for d in range(3)]
            if any(x0 > x1 for x0, x1 in cut):                 # the box misses the cube: both states stay as drawn
                assert dyadic and kind != "d0"
                olds.append(so), news.append(sn), cubes.append(None)
                continue
            sl = tuple(slice(cut[a][0] - lo[a], cut[a][1] - lo[a] + 1) for a in (2, 1, 0))
            m = so[0][sl].shape
            if kind in ("+", "-"):
                sn[0][sl] = so[0][sl] + (1.0 if kind == "+" else -1.0) * rng.uniform(-0.1, 0.4, size=m)
            elif kind == "0":
                sn[0][sl] = so[0][sl]
            else:
                span = {"d+": (-8, 25), "d-": (-24, 9), "d0": (-16, 17), "d-+": ((-24, 0), (8, 41))[min(b, 1)]}[kind]
                sn[0][sl] = so[0][sl] + rng.integers(span[0], span[1], size=m) / 64.0
            olds.append(so), news.append(sn), cubes.append(sl)
        if kind == "d0":                    # the last cube zone of the last box takes what is left: the parts cancel exactly
            total = sum(float((n[0][s] - o[0][s]).sum()) for o, n, s in zip(olds, news, cubes))
            last = tuple(x.stop - 1 for x in cubes[-1])
            news[-1][0][last] -= total
            assert news[-1][0][last] > 0.0 and sum(float((n[0][s] - o[0][s]).sum()) for o, n, s in zip(olds, news, cubes)) == 0.0
        for b in range(len(boxes)):
            A[P + "sold%d" % b], A[P + "snew%d" % b] = olds[b], news[b]


def save_npz(path, arrays):
    """np.savez_compressed without the clock: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type, zi.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zi, buf.getvalue())


def source_vectors(exe, tmp, dst):
    rng = np.random.default_rng(20261018)
    A = {}
    sponge_inputs(rng, A)
    gravity_inputs(rng, A)
    pointmass_inputs(rng, A)
    A = {k: np.atleast_1d(np.asarray(v, dtype=np.float64)) for k, v in A.items()}
    write_blob(os.path.join(tmp, "in5.bin"), A)
    subprocess.check_call([exe + "_sources", os.path.join(tmp, "in5.bin"), os.path.join(tmp, "out5.bin")])
    O = read_blob(os.path.join(tmp, "out5.bin"))
    shaped = {}
    for k, v in O.items():
        P, name = k.split(".")
        if name in ("src", "old", "new"):
            lo, hi = [int(x) for x in A[P + ".box"][:3]], [int(x) for x in A[P + ".box"][3:]]
            v = v.reshape((7,) + _shape(lo, hi))
        elif name.startswith("snew"):
            v = v.reshape(A[P + "." + name].shape)
        shaped["out:" + k] = v
    allv = {"in:" + k: v for k, v in A.items()}
    allv.update(shaped)
    path = os.path.join(dst, "source_vectors.npz")
    save_npz(path, allv)
    print("wrote %s: %d input arrays, %d output arrays, %.1f KB" % (path, len(A), len(O), os.path.getsize(path) / 1024.0))
    for fam in ("sponge", "grav", "pm"):
        print("  %-8s %8d recorded values" % (fam, sum(v.size for k, v in shaped.items() if k.startswith("out:" + fam))))


# ---- the boundary overrides: bc<c>.* of tests/golden/stub_probe/bc_vectors.npz -------------------------------------------------
# FAB boxes: the two of the source-term fixture.  cut: {(direction, side): n} -- that face of the domain cuts the FAB n zones in;
# every other face lies 10 zones outside the FAB.  bc: {(direction, side): physical boundary}, Outflow where not named
INTERIOR, INFLOW, OUTFLOW, SYMMETRY, SLIPWALL = 0, 1, 2, 3, 4
_BOX_A, _BOX_B = (SRC_BOXES[0]["lo"], SRC_BOXES[0]["hi"]), (SRC_BOXES[1]["lo"], SRC_BOXES[1]["hi"])
_XL, _XR, _YL, _YR, _ZL, _ZR = (0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)
_ALL6 = {_XL: 2, _XR: 2, _YL: 2, _YR: 2, _ZL: 1, _ZR: 1}
_ZLOW = dict(box=_BOX_B, cut={_ZL: 4, _XL: 1}, bc={_ZL: INFLOW, _XL: SLIPWALL}, hse=[_ZL])      # with a ghost row beyond an x wall
_XLOW = dict(box=_BOX_A, cut={_XL: 4, _YR: 1}, bc={_XL: INFLOW, _YR: SYMMETRY}, hse=[_XL])
BC_CASES = [
    dict(_XLOW),                                                                        # 0-4: each of the five HSE faces alone
    dict(box=_BOX_A, cut={_XR: 4}, bc={_XR: INFLOW}, hse=[_XR]),
    dict(box=_BOX_A, cut={_YL: 4}, bc={_YL: INFLOW}, hse=[_YL]),
    dict(box=_BOX_A, cut={_YR: 4, _ZL: 1}, bc={_YR: INFLOW, _ZL: SLIPWALL}, hse=[_YR]),
    dict(_ZLOW),
    dict(box=_BOX_A, cut={_XL: 4, _XR: 4}, bc={_XL: INFLOW, _XR: INFLOW}, hse=[_XL, _XR]),     # 5: x low and x high together
    dict(_ZLOW, hse_zero_vels=1), dict(_ZLOW, hse_reflect_vels=1), dict(_ZLOW, hse_interp_temp=1, temp=1.7e-8),      # 6-8
    dict(_XLOW, hse_zero_vels=1), dict(_XLOW, hse_reflect_vels=1), dict(_XLOW, hse_interp_temp=1, temp=0.9e-8),      # 9-11
    dict(_ZLOW, const_grav=-21.3, temp=1.2e-8),             # 12: a scale height of 3/4 dx: a density ratio of 5 per zone under the 10 % clamp
    dict(_ZLOW, const_grav=0.0),                            # 13
    dict(box=_BOX_A, cut={}, bc={_ZL: INFLOW}, hse=[_ZL]),                              # 14: the FAB does not reach the boundary
    dict(box=_BOX_B, cut={_ZL: 1}, bc={_ZL: INFLOW}, hse=[_ZL]),                        # 15: one ghost layer (four: case 4)
    dict(box=_BOX_A, cut=_ALL6, bc={}, fill_ambient_bc=1, ambient_fill_dir=-1),         # 16-19: ambient alone; edges beyond two faces
    dict(box=_BOX_A, cut=_ALL6, bc={}, fill_ambient_bc=1, ambient_fill_dir=0),
    dict(box=_BOX_A, cut=_ALL6, bc={}, fill_ambient_bc=1, ambient_fill_dir=1),
    dict(box=_BOX_A, cut=_ALL6, bc={}, fill_ambient_bc=1, ambient_fill_dir=2),
    dict(box=_BOX_A, cut=_ALL6, bc={_XL: INFLOW, _XR: SLIPWALL}, fill_ambient_bc=1),    # 20: a wall and an Inflow face stay as they are
    dict(box=_BOX_A, cut=_ALL6, bc={}, fill_ambient_bc=1, ambient_outflow_vel=1),       # 21: both signs on low and high faces, edges
    dict(box=_BOX_A, cut=_ALL6, bc={_XL: SLIPWALL, _XR: SYMMETRY, _ZL: INTERIOR, _ZR: INTERIOR}, fill_ambient_bc=1,
         ambient_outflow_vel=1),                                                        # 22: edge zones beyond an ambient face and a wall
    dict(box=_BOX_B, cut={_ZL: 4, _ZR: 2, _XL: 1}, bc={_ZL: INFLOW, _XL: SLIPWALL}, hse=[_ZL], fill_ambient_bc=1, ambient_fill_dir=2,
         ambient_outflow_vel=1),                                                        # 23: ambient on +z, HSE on z low
    dict(box=_BOX_B, cut={_ZL: 4, _XL: 1}, bc={_ZL: INFLOW}, hse=[_ZL], fill_ambient_bc=1),     # 24: an HSE column that starts from an ambient zone
    dict(box=_BOX_B, cut={_ZL: 4, _YR: 1}, bc={_ZL: INFLOW}, hse=[_ZL], hse_reflect_vels=1, fill_ambient_bc=1, ambient_outflow_vel=1),
    # 26: temperatures a decade apart from zone to zone, extrapolated below zero in some columns: their Newton loops run out.  The
    # reference's CPU build aborts there, its GPU build says nothing: this case runs in the executable whose hse_fill.cpp saw
    # -DAMREX_USE_GPU (the abort is the only thing the macro touches in the two files and the headers they include)
    dict(_ZLOW, hse_interp_temp=1, silent=True),
]
BC_AMBIENT = dict(ambient_density=0.01372918, ambient_temp=3.1871e-9, ambient_energy=0.6172839)
BC_SMALL = dict(small_dens=1.e-6, small_temp=1.e-12, small_ener=1.e-9)


def generic_fill(U, lo, hi, domlo, domhi, lo_bc, hi_bc):
    """the generic physical-boundary fill (first-order extrapolation, Inflow included; mirrors with the normal momentum negated
    at the walls): every zone outside the domain from the zone inside it that the three sweeps compose to"""
    idx, flip = [], []
    for d in range(3):
        i = np.arange(lo[d], hi[d] + 1)
        s, f = i.copy(), np.zeros(i.size, dtype=bool)
        for side, bc in ((0, lo_bc[d]), (1, hi_bc[d])):
            out = i < domlo[d] if side == 0 else i > domhi[d]
            edge = domlo[d] if side == 0 else domhi[d]
            if bc in (INFLOW, OUTFLOW):
                s[out] = edge
            elif bc >= SYMMETRY:
                s[out] = 2 * edge - i[out] + (-1 if side == 0 else 1)
                f |= out
        idx.append(s - lo[d]), flip.append(f)
    V = U[:, idx[2][:, None, None], idx[1][None, :, None], idx[0][None, None, :]].copy()
    for d, ax in enumerate((2, 1, 0)):
        shape = [1, 1, 1]
        shape[ax] = -1
        V[1 + d] = np.where(flip[d].reshape(shape), -V[1 + d], V[1 + d])
    return V


def bc_inputs(rng, A):
    for c, case in enumerate(BC_CASES):
        P = "bc%d." % c
        lo, hi = case["box"]
        shp = _shape(lo, hi)
        domlo, domhi = [x - 10 for x in lo], [x + 10 for x in hi]
        for (d, side), n in case["cut"].items():
            if side == 0:
                domlo[d] = lo[d] + n
            else:
                domhi[d] = hi[d] - n
        lo_bc, hi_bc = [OUTFLOW] * 3, [OUTFLOW] * 3
        for (d, side), bc in case["bc"].items():
            (lo_bc if side == 0 else hi_bc)[d] = bc
        types = [-1.0] * 6
        for d, side in case.get("hse", []):
            types[2 * d + side] = 1.0
        rho = 10.0 ** rng.uniform(-1.0, 1.0, shp)
        T = 10.0 ** rng.uniform(-8.5, -7.5, shp) if "temp" not in case else case["temp"] * rng.uniform(0.95, 1.05, shp)
        U = np.zeros((8,) + shp)
        U[0], U[6], U[7] = rho, T, rho * rng.uniform(0.9, 1.0, shp)
        for k in range(3):
            U[1 + k] = rho * rng.normal(size=shp)
        U[5] = rho * (K_B * T / ((GAMMA - 1.0) * M_U))
        U[4] = U[5] + 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / rho
        A[P + "U"] = generic_fill(U, lo, hi, domlo, domhi, lo_bc, hi_bc)
        A[P + "box"], A[P + "dx"] = np.array(lo + hi, dtype=np.float64), SRC_DX
        A[P + "domlo"], A[P + "domhi"], A[P + "lo_bc"], A[P + "hi_bc"] = domlo, domhi, lo_bc, hi_bc
        A[P + "types"] = types
        A[P + "flags"] = [case.get(k, v) for k, v in (("hse_zero_vels", 0), ("hse_interp_temp", 0), ("hse_reflect_vels", 0),
                                                      ("fill_ambient_bc", 0), ("ambient_fill_dir", -1), ("ambient_outflow_vel", 0))]
        A[P + "const_grav"], A[P + "eos_gamma"], A[P + "silent"] = case.get("const_grav", -1.0), GAMMA, float(bool(case.get("silent")))
        # ambient::ambient_state (Castro_setup.cpp:339-350)
        dens = max(BC_AMBIENT["ambient_density"], BC_SMALL["small_dens"])
        rhoe = dens * max(BC_AMBIENT["ambient_energy"], BC_SMALL["small_ener"])
        A[P + "ambient"] = [dens, 0.0, 0.0, 0.0, rhoe, rhoe, max(BC_AMBIENT["ambient_temp"], BC_SMALL["small_temp"]), dens * (1.0 / 1)]
        for k, v in dict(BC_AMBIENT, **BC_SMALL).items():
            A[P + k] = v


def bc_vectors(exe, tmp, dst):
    rng = np.random.default_rng(20261019)
    A = {}
    bc_inputs(rng, A)
    A = {k: np.atleast_1d(np.asarray(v, dtype=np.float64)) for k, v in A.items()}
    silent = tuple("bc%d." % c for c, case in enumerate(BC_CASES) if case.get("silent"))
    O = {}
    for tag, suffix, keep in (("in6", "_bc", lambda k: not k.startswith(silent)), ("in7", "_bc_silent", lambda k: k.startswith(silent))):
        write_blob(os.path.join(tmp, tag + ".bin"), {k: v for k, v in A.items() if keep(k)})
        subprocess.check_call([exe + suffix, os.path.join(tmp, tag + ".bin"), os.path.join(tmp, tag + ".out")])
        O.update(read_blob(os.path.join(tmp, tag + ".out")))
    allv = {"in:" + k: v for k, v in A.items()}
    for k, v in O.items():
        allv["out:" + k] = v.reshape(A[k].shape)
    path = os.path.join(dst, "bc_vectors.npz")
    save_npz(path, allv)
    print("wrote %s: %d input arrays, %d output arrays, %.1f KB" % (path, len(A), len(O), os.path.getsize(path) / 1024.0))
    for k in sorted(O, key=lambda s: int(s[2:].split(".")[0])):
        changed = int((allv["out:" + k].view(np.int64) != A[k].view(np.int64)).any(axis=0).sum())
        print("  %-8s %6d zones, %5d changed, %d NaN" % (k, A[k][0].size, changed, int(np.isnan(O[k]).sum())))


def edge_states(rng, n, gam=1.4, cold=0.15):
    """(7, n) edge states (rho,u,v,w,p,rhoe,X): jumps of many decades, supersonic flows, some with rho e <= 0 or a tiny
    pressure (the EOS clean-up of load_input_states)"""
    rho = 10.0 ** rng.uniform(-3, 2, n)
    vel = rng.normal(size=(3, n)) * 10.0 ** rng.uniform(-2, 1, n)
    p = 10.0 ** rng.uniform(-5, 3, n)
    rhoe = p / (gam - 1.0) * rng.choice([1.0, 1.0, 1.0, 0.6, 2.5], n)
    bad = rng.uniform(size=n) < cold * 0.2
    rhoe = np.where(bad, -rhoe, rhoe)
    X = rng.uniform(size=n)
    return np.stack([rho, vel[0], vel[1], vel[2], p, rhoe, X])


def flux_records(rng, n):
    """(9, n): rho, mx, my, mz, E, X fluxes, Godunov un, Godunov p, (rho e) flux"""
    f = rng.normal(size=(9, n)) * 10.0 ** rng.uniform(-2, 1, n)
    f[7] = 10.0 ** rng.uniform(-4, 2, n)
    return f


def main():
    rng = np.random.default_rng(20211007)
    A = {}
    # ---- ppm ----
    n = 6000
    kind = rng.integers(0, 5, n)
    x = rng.uniform(0, 6.3, n)
    s = np.empty((5, n))
    for m in range(5):
        smooth = np.sin(x + 0.4 * m) + 2.0
        noisy = rng.normal(size=n)
        mono = np.cumsum(rng.uniform(0, 1, (5, n)), axis=0)[m]
        step = np.where(m < 2 + rng.integers(0, 2, n), 1.0, rng.uniform(0.01, 100.0, n))
        flat = np.full(n, 3.0) + (m == 2) * rng.choice([0.0, 1e-13], n)
        s[m] = np.choose(kind, [smooth, noisy, mono, step, flat])
    A["ppm.s"] = s
    A["ppm.flat"] = rng.choice([0.0, 1.0, 1.0, 0.37], n) * np.where(rng.uniform(size=n) < 0.2, rng.uniform(size=n), 1.0)
    A["ppm.u"] = rng.normal(scale=2.0, size=n)
    A["ppm.c"] = 10.0 ** rng.uniform(-2, 1, n)
    A["ppm.dtdx"] = 0.27
    # ---- flattening along one direction ----
    n = 4000
    base = 10.0 ** rng.uniform(-3, 2, n)
    p7 = base * (1.0 + 0.05 * rng.normal(size=(7, n)))
    jump = rng.integers(0, 8, n)
    for m in range(7):
        p7[m] = np.where(m >= jump, p7[m] * rng.choice([1.0, 1.5, 4.0, 50.0, 0.02], n), p7[m])
    A["flat.p"] = np.abs(p7)
    A["flat.u"] = rng.normal(size=(5, n)) + np.linspace(1.5, -1.5, 5)[:, None] * rng.choice([0.0, 1.0, -1.0], n)
    # ---- cmpflx_plus_godunov ----
    cfgs = [dict(idir=0), dict(idir=1), dict(idir=2, wall=1), dict(idir=0, riemann_solver=1, cg_blend=2),
            dict(idir=1, riemann_solver=1, cg_blend=1), dict(idir=2, riemann_solver=1, cg_blend=1, wall=1),
            dict(idir=0, riemann_solver=2), dict(idir=2, riemann_solver=2, wall=1), dict(idir=0, hybrid_riemann=1),
            dict(idir=1, riemann_solver=2, hybrid_riemann=1), dict(idir=1, small_pres=1e-4, small_dens=1e-2),
            dict(idir=2, riemann_solver=1, cg_blend=2, small_pres=1e-4)]
    for c, cfg in enumerate(cfgs):
        n = 450
        P = "cmpflx%d." % c
        qm, qp = edge_states(rng, n), edge_states(rng, n)
        same = rng.uniform(size=n) < 0.15
        qp[:, same] = qm[:, same] * (1.0 + 1e-3 * rng.normal(size=(7, int(same.sum()))))
        qp[0] = np.abs(qp[0]); qp[4] = np.abs(qp[4])
        cz = 10.0 ** rng.uniform(-2, 1.5, n + 1)
        A[P + "qm"], A[P + "qp"], A[P + "c"] = qm, qp, cz
        A[P + "shk"] = (rng.uniform(size=n + 1) < 0.3).astype(float) if cfg.get("hybrid_riemann") else np.zeros(n + 1)
        A[P + "wall"] = float(cfg.get("wall", 0))
        for k, v in cfg.items():
            if k != "wall":
                A[P + k] = float(v)
    # ---- trans_single ----
    tcfgs = [dict(idir_t=0, idir_n=1), dict(idir_t=1, idir_n=0), dict(idir_t=2, idir_n=0), dict(idir_t=0, idir_n=2),
             dict(idir_t=1, idir_n=2), dict(idir_t=2, idir_n=1), dict(idir_t=0, idir_n=1, transverse_reset_density=0),
             dict(idir_t=1, idir_n=2, transverse_reset_rhoe=1), dict(idir_t=2, idir_n=0, transverse_use_eos=1)]
    for c, cfg in enumerate(tcfgs):
        n = 500
        P = "trans1_%d." % c
        q = edge_states(rng, n, cold=0.0)
        q[5] = np.abs(q[5])
        A[P + "q"] = q
        A[P + "flux"] = flux_records(rng, n + 1) * rng.choice([1.0, 1.0, 30.0], n + 1)     # some large enough to flip the density
        A[P + "qt"] = np.zeros(1)
        A[P + "cdtdx"] = 0.011
        for k, v in cfg.items():
            A[P + k] = float(v)
    # ---- trans_final ----
    fcfgs = [dict(idir_n=0, idir_t1=1, idir_t2=2), dict(idir_n=1, idir_t1=0, idir_t2=2), dict(idir_n=2, idir_t1=0, idir_t2=1),
             dict(idir_n=0, idir_t1=1, idir_t2=2, transverse_reset_density=0), dict(idir_n=2, idir_t1=0, idir_t2=1, transverse_reset_rhoe=1)]
    for c, cfg in enumerate(fcfgs):
        n = 500
        P = "trans2_%d." % c
        q = edge_states(rng, n, cold=0.0)
        q[5] = np.abs(q[5])
        A[P + "q"] = q
        A[P + "flux1"] = flux_records(rng, n + 1) * rng.choice([1.0, 1.0, 20.0], n + 1)
        A[P + "flux2l"] = flux_records(rng, n)
        A[P + "flux2r"] = flux_records(rng, n) * rng.choice([1.0, 1.0, 20.0], n)
        A[P + "cdtdx1"], A[P + "cdtdx2"] = 0.017, 0.013
        for k, v in cfg.items():
            A[P + k] = float(v)
    # ---- a block through ctoprim, uflatten, trace_ppm ----
    nb = 6
    U = physical_state(rng, (-4, -4, -4), (nb + 3, nb + 3, nb + 3), smooth=False, vel=1.5, jump=True)
    A["block.U"], A["block.n"], A["block.dt"], A["block.dx"] = U, float(nb), 7.0e-4, np.array([0.02, 0.025, 0.03])

    # ---- whole tiles of construct_ctu_hydro_source (probe.cpp drives the reference's own functions) ----
    nb = 6
    glo, ghi = (-4, -4, -4), (nb + 3, nb + 3, nb + 3)
    floors = dict(small_dens=1e-8, small_pres=1e-10, small_temp=1e-10, small_ener=1e-12)
    hcfgs = [dict(), dict(riemann_solver=1, cg_blend=2), dict(riemann_solver=2, ppm_type=0), dict(hybrid_riemann=1),
             dict(ppm_temp_fix=2), dict(transverse_reset_rhoe=1, transverse_use_eos=1, transverse_reset_density=0),
             dict(limit_fluxes_on_small_dens=1, limit_fluxes_on_large_vel=1, speed_limit=2.0, small_dens=0.1, cfl=0.5),
             dict(wall_lo=1), dict(src=1), dict(src=1, ppm_type=0, source_term_predictor=1, corr=1, use_pslope=1),
             dict(first_order_hydro=1), dict(use_flattening=0, difmag=0.0, riemann_solver=1, cg_blend=1),
             dict(ppm_type=0, plm_iorder=1), dict(ppm_type=0, plm_limiter=1, hybrid_riemann=1, riemann_solver=2)]
    for c, cfg in enumerate(hcfgs):
        P = "hydro%d." % c
        U = physical_state(rng, glo, ghi, smooth=(c % 3 == 0), vel=1.5 if c % 2 else 0.7, jump=True)
        if cfg.get("wall_lo"):                      # reflect the ghost zones below index 0 like a SlipWall fill would
            for d, ax in enumerate((3, 2, 1)):
                idx = [slice(None)] * 4
                for g in range(4):
                    src_i, dst_i = list(idx), list(idx)
                    src_i[ax], dst_i[ax] = 4 + g, 3 - g
                    U[tuple(dst_i)] = U[tuple(src_i)]
                    U[(1 + d,) + tuple(dst_i[1:])] *= -1.0
        A[P + "U"], A[P + "n"], A[P + "dt"], A[P + "dx"] = U, float(nb), 6.0e-3, np.array([0.05, 0.055, 0.045])
        if cfg.get("src"):
            S = np.zeros((7,) + U.shape[1:])
            g = np.array([0.3, -9.0, 1.5])
            for d in range(3):
                S[1 + d] = U[0] * g[d]
                S[4] += U[1 + d] * g[d]
            A[P + "src"] = S
        if cfg.get("corr"):
            A[P + "corr"] = 0.4 * A[P + "src"] * rng.uniform(0.5, 1.5, size=A[P + "src"].shape)
        for k, v in dict(floors, **cfg).items():
            if k not in ("src", "corr"):
                A[P + k] = float(v)

    # ---- problem initialisers: Exec/hydro_tests/Sedov and Sod (problem_initialize + problem_initialize_state_data) ----
    B = {}
    sed = [dict(n=(16, 16, 16), problo=(0., 0., 0.), probhi=(1., 1., 1.), r_init=0.01, p_ambient=1.e-5, exp_energy=1.0, dens_ambient=1.0, nsub=10),
           dict(n=(12, 10, 14), problo=(-0.5, 0., 0.25), probhi=(0.7, 1.1, 1.3), r_init=0.2, p_ambient=1.e-3, exp_energy=2.5, dens_ambient=0.7, nsub=4),
           dict(n=(8, 8, 8), problo=(0., 0., 0.), probhi=(1., 1., 1.), r_init=0.3, p_ambient=1.e-5, exp_energy=1.0, dens_ambient=1.0, nsub=5)]
    for c, cfg in enumerate(sed):
        for k, v in cfg.items():
            B["sedov%d.%s" % (c, k)] = np.atleast_1d(np.asarray(v, dtype=np.float64))
    sod = [dict(n=(32, 4, 4), problo=(0., 0., 0.), probhi=(1., 0.125, 0.125), idir=1, frac=0.5, left=(1.0, 0.0, 1.0), right=(0.125, 0.0, 0.1)),
           dict(n=(4, 24, 4), problo=(0.1, -0.2, 0.), probhi=(0.35, 1.3, 0.25), idir=2, frac=0.3, left=(1.0, 0.75, 1.0), right=(0.125, -2.0, 0.4)),
           dict(n=(4, 6, 20), problo=(0., 0., 0.), probhi=(0.2, 0.3, 1.0), idir=3, frac=0.5, left=(5.99924, 19.5975, 460.894), right=(5.99242, -6.19633, 46.0950))]
    for c, cfg in enumerate(sod):
        for k, v in cfg.items():
            B["sod%d.%s" % (c, k)] = np.atleast_1d(np.asarray(v, dtype=np.float64))

    dst = os.path.join(ROOT, "tests", "golden", "stub_probe")
    os.makedirs(dst, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        write_blob(os.path.join(tmp, "in.bin"), A)
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
        O = read_blob(os.path.join(tmp, "out.bin"))
        write_blob(os.path.join(tmp, "in2.bin"), B)
        subprocess.check_call([exe + "_init", os.path.join(tmp, "in2.bin"), os.path.join(tmp, "out2.bin")])
        O.update(read_blob(os.path.join(tmp, "out2.bin")))
        # ---- derived fields on one box (state with one ghost zone for the vorticity and the divergence) ----
        dn = (10, 9, 8)
        D = {"derive.n": np.array(dn, dtype=np.float64), "derive.dx": np.array([0.05, 0.04, 0.0625]), "derive.problo": np.array([-0.2, 0.1, 0.0]),
             "derive.center": np.array([0.05, 0.28, 0.25]),
             "derive.U": physical_state(rng, (-1, -1, -1), dn, smooth=False, vel=1.5, jump=True)}
        write_blob(os.path.join(tmp, "in3.bin"), D)
        subprocess.check_call([exe + "_derive", os.path.join(tmp, "in3.bin"), os.path.join(tmp, "out3.bin")])
        for k, v in read_blob(os.path.join(tmp, "out3.bin")).items():
            if k == "derive.estdt":
                O[k] = v
                continue
            nc = v.size // ((dn[0] + 2) * (dn[1] + 2) * (dn[2] + 2))
            O[k] = v.reshape(nc, dn[2] + 2, dn[1] + 2, dn[0] + 2)[:, 1:-1, 1:-1, 1:-1].copy()
        B.update(D)
        # ---- rotation sources: rsrc on the old state, corrrsrc with old and new state and the mass fluxes ----
        R = {}
        rn = (7, 6, 5)
        rcfg = [dict(axis=3, rot_source_type=4, implicit=1, centrifugal=1, coriolis=1), dict(axis=1, rot_source_type=1, implicit=0, centrifugal=1, coriolis=1),
                dict(axis=2, rot_source_type=2, implicit=1, centrifugal=0, coriolis=1), dict(axis=3, rot_source_type=3, implicit=1, centrifugal=1, coriolis=0),
                dict(axis=3, rot_source_type=4, implicit=0, centrifugal=1, coriolis=1), dict(axis=1, rot_source_type=3, implicit=0, centrifugal=1, coriolis=1)]
        for c, cfg in enumerate(rcfg):
            P = "rot%d." % c
            R[P + "n"], R[P + "dx"], R[P + "problo"] = np.array(rn, dtype=np.float64), np.array([0.1, 0.12, 0.15]), np.array([-0.3, 0.0, 0.2])
            R[P + "center"], R[P + "period"], R[P + "dt"] = np.array([0.05, 0.36, 0.55]), np.array([2.5]), np.array([0.02])
            hi = tuple(x - 1 for x in rn)
            R[P + "uold"] = physical_state(rng, (0, 0, 0), hi, smooth=False, vel=1.5, jump=True)
            R[P + "unew"] = R[P + "uold"] * rng.uniform(0.9, 1.1, size=R[P + "uold"].shape)
            for d in range(3):
                shp = [rn[2], rn[1], rn[0]]
                shp[2 - d] += 1
                R[P + "mflux%d" % d] = rng.normal(scale=1e-4, size=shp)
            for k, v in cfg.items():
                R[P + k] = np.array([float(v)])
        write_blob(os.path.join(tmp, "in4.bin"), R)
        subprocess.check_call([exe + "_rotation", os.path.join(tmp, "in4.bin"), os.path.join(tmp, "out4.bin")])
        O.update(read_blob(os.path.join(tmp, "out4.bin")))
        B.update(R)
        source_vectors(exe, tmp, dst)
        bc_vectors(exe, tmp, dst)
    A.update(B)
    # whole-tile outputs: keep the zones and faces the call defines (everything lives on the box grown by 4 in the probe)
    m = nb + 8
    for c in range(len(hcfgs)):
        P = "hydro%d." % c
        O[P + "unew"] = O[P + "unew"].reshape(8, m, m, m)[:, 4:4 + nb, 4:4 + nb, 4:4 + nb].copy()
        for d in range(3):
            sl = [slice(4, 4 + nb + (1 if ax == d else 0)) for ax in (2, 1, 0)]
            O[P + "flux%d" % d] = O[P + "flux%d" % d].reshape(8, m, m, m)[(slice(None),) + tuple(sl)].copy()
            O[P + "qe%d" % d] = O[P + "qe%d" % d].reshape(4, m, m, m)[(slice(None),) + tuple(sl)].copy()
        for k in ("div", "shk", "srcq"):
            O.pop(P + k)
    allv = {"in:" + k: np.atleast_1d(np.asarray(v, dtype=np.float64)) for k, v in A.items()}
    allv.update({"out:" + k: v for k, v in O.items()})
    # np.savez_compressed stamps every member with the clock, so a file written again never has the bytes of the last one:
    # vectors.npz is written only where its arrays changed (or it is missing), and is otherwise left as it is
    path = os.path.join(dst, "vectors.npz")
    if os.path.exists(path):
        with np.load(path) as old:
            same = sorted(old.files) == sorted(allv) and all(
                old[k].shape == allv[k].shape and np.array_equal(old[k].view(np.int64), allv[k].view(np.int64)) for k in allv)
    else:
        same = False
    if same:
        print("%s: every array reproduced bit for bit, file left as it is" % path)
    else:
        np.savez_compressed(path, **allv)
        print("wrote %s: %d input arrays, %d output arrays, %.1f KB" % (path, len(A), len(O), os.path.getsize(path) / 1024.0))
    for k in sorted(O):
        print("  %-16s %8d values, %d NaN" % (k, O[k].size, int(np.isnan(O[k]).sum())))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/stub_probe/multipole_vectors.npz: inputs and outputs of calcLegPolyL, calcAssocLegPolyLM and
multipole_add of the reference's Source/gravity/Gravity_util.H.

STUB-COMPILED, NOT a reference build (tools/stub_probe/README.md): probe_multipole.cpp includes the header unmodified and in
place, against the stand-in headers of stub/ with -DPROBE_MULTIPOLE.  Nothing of the reference's text is copied: the committed
artefacts are this recipe and the vectors (data, no time stamps: the same arrays give the same bytes).

Zones: on the z axis (cosTheta = 1 and -1, x = y = 0), in the plane y = 0 on both sides of the axis (phiAngle = 0 and pi), in the
plane z = 0 (cosTheta = 0), and in general position; r from 1e-3 to 1 (distances are divided by rmax); rho and vol with full
mantissas.  r, cosTheta and phiAngle are formed as Gravity::fill_multipole_BCs forms them (Gravity.cpp:1910-1918) and recorded,
so a replay starts from the arguments the reference's functions were given."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CASTRO_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)
from make_vectors import save_npz   # noqa: E402

LNUMS = (0, 2, 6)


def zones(rng):
    g = rng.uniform(-1.0, 1.0, size=(40, 3)) * rng.choice([1.0, 0.3, 0.01], size=(40, 1))
    special = np.array([[0.0, 0.0, 0.37], [0.0, 0.0, -0.81], [0.0, 0.0, 1.0e-3],          # on the z axis: cosTheta = +-1
                        [0.42, 0.0, 0.13], [-0.42, 0.0, 0.13], [0.9, 0.0, -0.2],          # y = 0: phiAngle = 0 or pi
                        [0.3, 0.4, 0.0], [-0.25, -0.6, 0.0],                              # z = 0: cosTheta = 0
                        [0.0, 0.55, 0.2], [0.0, -0.55, -0.2]])                            # x = 0: phiAngle = +-pi / 2
    xyz = np.concatenate([special, g])
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r = np.sqrt(x * x + y * y + z * z)
    cos_theta = z / r
    phi = np.arctan2(y, x)
    rho = rng.uniform(0.1, 10.0, size=r.size) * 10.0 ** rng.integers(-3, 9, size=r.size)
    vol = rng.uniform(1.0e-6, 1.0e-3, size=r.size)
    return np.stack([cos_theta, phi, r, rho, vol], axis=1)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "probe_multipole")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DPROBE_MULTIPOLE",
                               "-I" + os.path.join(HERE, "stub"), "-I" + os.path.join(REF, "Source", "gravity"),
                               os.path.join(HERE, "probe_multipole.cpp"), "-o", exe])
        Z = zones(np.random.default_rng(20211))
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        np.concatenate([[float(Z.shape[0])], Z.reshape(-1)]).astype(np.float64).tofile(fin)
        subprocess.check_call([exe, fin, fout])
        out = np.fromfile(fout, dtype=np.float64)
    A = {"zones": Z}
    at = 0
    for lnum in LNUMS:
        n1 = lnum + 1
        per = n1 + n1 * n1 + n1 + 2 * n1 * n1
        blk = out[at:at + per * Z.shape[0]].reshape(Z.shape[0], per)
        at += per * Z.shape[0]
        o = 0
        for name, size, shape in (("leg", n1, (n1,)), ("assoc", n1 * n1, (n1, n1)), ("qL0", n1, (n1,)),
                                  ("qLC", n1 * n1, (n1, n1)), ("qLS", n1 * n1, (n1, n1))):
            A["l%d.%s" % (lnum, name)] = blk[:, o:o + size].reshape((Z.shape[0],) + shape)
            o += size
    assert at == out.size
    dst = os.path.join(ROOT, "tests", "golden", "stub_probe", "multipole_vectors.npz")
    save_npz(dst, A)
    print("wrote %s: %d zones, %d bytes" % (dst, Z.shape[0], os.path.getsize(dst)))


if __name__ == "__main__":
    main()

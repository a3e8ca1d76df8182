"""Reference for the integrated quantities (castro_amd_integrated_quantities_mf), tests only.

Per zone the terms are the CPU oracle's derived fields for kineng and angular_momentum_* (ora_derive), the state components
themselves for the rest, and loc_d = problo_d + (0.5 + index_d) * dx_d; each is multiplied by vol = dx dy dz in double, zones
under a zero mask byte are dropped, and every quantity is the exactly rounded sum math.fsum of its terms.

Tolerance (derived, not tuned).  Any order of N double additions is within (N - 1) * 2**-53 * A of the exact sum to first order,
A = fsum(|t_i|).  `exact` build: the terms are the oracle's bits, so the bound is N * 2**-52 * A (the factor 2 absorbs the second
order).  `contract` build: the terms may differ by contraction; the project's contract criterion (1e-10 relative to the largest
magnitude of the field) applied per zone adds 1e-10 * N * vol * max|field|, where for the angular momenta the field is measured
against |loc - c| * |rho u| (the cross product cancels).
"""
import ctypes as C
import math

import numpy as np

DIAG_N = 14
NAMES = ("mass", "xmom", "ymom", "zmom", "angmom_x", "angmom_y", "angmom_z", "rho_e", "rho_K", "rho_E", "com_x", "com_y", "com_z",
         "species")
URHO, UMX, UMY, UMZ, UEDEN, UEINT, UTEMP, UFS = range(8)
DER_KINENG, DER_ANGMOM_X = 1, 22


def _ora_derive(O, which, U, lo, geom, params, center):
    hi = tuple(lo[d] + U.shape[3 - d] - 1 for d in range(3))
    out = np.zeros((1,) + U.shape[1:])
    Uc = np.ascontiguousarray(U)               # kept alive over the call: the descriptor holds a bare pointer
    ctr = (C.c_double * 3)(*[float(x) for x in center])
    rc = O.lib().ora_derive(which, O.i3(lo), O.i3(hi), O.a4(Uc, lo, hi), O.a4(out, lo, hi),
                            C.byref(geom), C.byref(params), C.byref(ctr))
    assert rc == 0
    return out[0]


def zone_terms(O, U, lo, geom, params, center):
    """(terms, scale): 14 arrays (nz, ny, nx) of per-zone terms already multiplied by vol, and 14 arrays of the magnitude the
    contract criterion measures each field against.  U: the valid zones (8, nz, ny, nx) of the box starting at lo."""
    nz, ny, nx = U.shape[1:]
    dx = [geom.dx[d] for d in range(3)]
    vol = dx[0] * dx[1] * dx[2]
    loc = [geom.problo[d] + (0.5 + np.arange(lo[d], lo[d] + n, dtype=np.float64)) * dx[d] for d, n in enumerate((nx, ny, nz))]
    X = [loc[0][None, None, :] + np.zeros((nz, ny, nx)), loc[1][None, :, None] + np.zeros((nz, ny, nx)),
         loc[2][:, None, None] + np.zeros((nz, ny, nx))]
    with np.errstate(all="ignore"):
        kin = _ora_derive(O, DER_KINENG, U, lo, geom, params, center)
        ang = [_ora_derive(O, DER_ANGMOM_X + d, U, lo, geom, params, center) for d in range(3)]
        fields = [U[URHO], U[UMX], U[UMY], U[UMZ], ang[0], ang[1], ang[2], U[UEINT], kin, U[UEDEN],
                  U[URHO] * X[0], U[URHO] * X[1], U[URHO] * X[2], U[UFS]]
        r = np.sqrt(sum((X[d] - center[d]) ** 2 for d in range(3)))
        pm = np.sqrt(U[UMX] ** 2 + U[UMY] ** 2 + U[UMZ] ** 2)
        scale = [np.abs(f) for f in fields]
        for d in range(3):
            scale[4 + d] = r * pm
        return [f * vol for f in fields], scale


def reference(O, boxes, geom, params, center):
    """boxes: [(U_valid (8, nz, ny, nx), lo, mask (nz, ny, nx) uint8 or None)].  Returns dict(S=[14 exactly rounded sums],
    A=[14 sums of |t_i|], N=contributing zones, fmax=[14 largest contract-criterion magnitudes], vol=zone volume)."""
    t_all = [[] for _ in range(DIAG_N)]
    f_all = [[] for _ in range(DIAG_N)]
    N = 0
    for U, lo, mask in boxes:
        terms, scale = zone_terms(O, U, lo, geom, params, center)
        keep = np.ones(U.shape[1:], dtype=bool) if mask is None else (np.asarray(mask) != 0)
        N += int(keep.sum())
        for m in range(DIAG_N):
            t_all[m].append(terms[m][keep])
            f_all[m].append(scale[m][keep])
    S, A, fmax = [], [], []
    for m in range(DIAG_N):
        t = np.concatenate(t_all[m]) if t_all[m] else np.zeros(0)
        f = np.concatenate(f_all[m]) if f_all[m] else np.zeros(0)
        S.append(math.fsum(t.tolist()))
        A.append(math.fsum(np.abs(t).tolist()))
        fmax.append(float(f.max()) if f.size else 0.0)
    return dict(S=S, A=A, N=N, fmax=fmax, vol=geom.dx[0] * geom.dx[1] * geom.dx[2])


def bounds(ref, numerics):
    """the tolerance of every quantity for a build of the kernel library ("exact" | "contract")"""
    b = [ref["N"] * 2.0 ** -52 * a for a in ref["A"]]
    if numerics == "contract":
        b = [x + 1e-10 * ref["N"] * ref["vol"] * f for x, f in zip(b, ref["fmax"])]
    return b


def numpy_sums(boxes, geom, center):
    """The 14 sums with numpy expressions (no oracle): the backend of the CPU driver tests and the hand-checked 4^3 case.
    boxes as for reference()."""
    out = np.zeros(DIAG_N)
    dx = [geom.dx[d] for d in range(3)]
    vol = dx[0] * dx[1] * dx[2]
    for U, lo, mask in boxes:
        nz, ny, nx = U.shape[1:]
        loc = [geom.problo[d] + (0.5 + np.arange(lo[d], lo[d] + n, dtype=np.float64)) * dx[d] for d, n in enumerate((nx, ny, nz))]
        X = [loc[0][None, None, :], loc[1][None, :, None], loc[2][:, None, None]]
        R = [X[d] - center[d] for d in range(3)]
        keep = np.ones((nz, ny, nx), dtype=bool) if mask is None else (np.asarray(mask) != 0)
        rho, mx, my, mz = U[URHO], U[UMX], U[UMY], U[UMZ]
        with np.errstate(all="ignore"):
            fields = [rho, mx, my, mz, R[1] * mz - R[2] * my, R[2] * mx - R[0] * mz, R[0] * my - R[1] * mx, U[UEINT],
                      0.5 / rho * (mx * mx + my * my + mz * mz), U[UEDEN], rho * X[0], rho * X[1], rho * X[2], U[UFS]]
            for m, f in enumerate(fields):
                out[m] += math.fsum(((f + np.zeros((nz, ny, nx))) * vol)[keep].tolist())
    return out

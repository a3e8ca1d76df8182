"""numpy restatement of the tracer-particle algorithms (castro_amd/csrc/tracer_kernels.hip; the issue's section 1), in the
expression order of the kernels: the cloud-in-cell gather, both passes of AdvectWithUcc, Redistribute, the sample and the count.
numpy evaluates every elementwise operation in IEEE double without contraction, so the device results are compared bit for bit.
Tests only.

Particles: a dict of numpy arrays x, y, z, r0, r1, r2 (float64) and id, cpu, level, grid (int32), updated in place.
Boxes of a level: [(fab, (alo, ahi), (vlo, vhi))] with fab shaped (ncomp, nz, ny, nx) over the array box [alo, ahi]."""
import numpy as np

URHO, UMX, UTEMP = 0, 1, 6
BIG = 1000000000


def particles(pos, level=0, grid=0):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    P = {k: np.zeros(n) for k in ("r0", "r1", "r2")}
    P["x"], P["y"], P["z"] = pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy()
    P["id"] = np.arange(1, n + 1, dtype=np.int32)
    P["cpu"] = np.zeros(n, dtype=np.int32)
    P["level"] = np.full(n, level, dtype=np.int32)
    P["grid"] = np.full(n, grid, dtype=np.int32)
    return P


def copy_particles(P):
    return {k: v.copy() for k, v in P.items()}


def tr_floor(l):
    """floor(l) as a zone index; what no int holds (NaN included) becomes +-10^9"""
    l = np.asarray(l, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        fl = np.floor(l)
        ok = np.abs(fl) < 1.0e9
        out = np.where(fl > 0.0, BIG, -BIG).astype(np.int64)
    out[ok] = fl[ok].astype(np.int64)
    return out


def dxi_of(geom):
    return [1.0 / geom.dx[d] for d in range(3)]


def _stencil_dir(pos, plo, dxi, alo, ahi):
    l = (pos - plo) * dxi - 0.5
    i = tr_floor(l)
    f = l - i.astype(np.float64)
    s = [1.0 - f, f]
    idx, clamped = [], np.zeros(pos.shape, dtype=bool)
    for q in range(2):
        c = i + q
        cc = np.clip(c, alo, ahi)
        clamped |= cc != c
        idx.append(cc - alo)
    return idx, s, clamped


def gather(fab, abox, geom, x, y, z, comp, vel=False):
    """(val, clamped) of component `comp` (vel: times 1 / rho) at the positions, all in the box whose array is `fab`"""
    alo, ahi = abox
    dxi = dxi_of(geom)
    ix, sx, cx = _stencil_dir(x, geom.problo[0], dxi[0], alo[0], ahi[0])
    iy, sy, cy = _stencil_dir(y, geom.problo[1], dxi[1], alo[1], ahi[1])
    iz, sz, cz = _stencil_dir(z, geom.problo[2], dxi[2], alo[2], ahi[2])
    val = np.zeros(x.shape)
    for kk in range(2):
        for jj in range(2):
            for ii in range(2):
                d = fab[comp][iz[kk], iy[jj], ix[ii]]
                if vel:
                    d = d * (1.0 / fab[URHO][iz[kk], iy[jj], ix[ii]])
                val = val + sx[ii] * sy[jj] * sz[kk] * d
    return val, cx | cy | cz


def _mine(P, level, nbox, flags):
    """[(box index, particle indices)] of the valid particles of `level`; a grid outside the table counts as a clamp"""
    sel = np.nonzero((P["id"] > 0) & (P["level"] == level))[0]
    g = P["grid"][sel]
    bad = (g < 0) | (g >= nbox)
    flags[0] += int(bad.sum())
    sel, g = sel[~bad], g[~bad]
    return [(b, sel[g == b]) for b in range(nbox) if (g == b).any()]


def advect_pass(P, level, boxes, geom, dt, ipass, flags):
    for b, t in _mine(P, level, len(boxes), flags):
        fab, abox, _ = boxes[b]
        x, y, z = P["x"][t], P["y"][t], P["z"][t]
        v, clamped = [], None
        for d in range(3):
            val, clamped = gather(fab, abox, geom, x, y, z, UMX + d, vel=True)
            v.append(val)
        flags[0] += int(clamped.sum())
        if ipass == 0:
            P["r0"][t], P["r1"][t], P["r2"][t] = x, y, z
            P["x"][t] = x + 0.5 * dt * v[0]
            P["y"][t] = y + 0.5 * dt * v[1]
            P["z"][t] = z + 0.5 * dt * v[2]
        else:
            P["x"][t] = P["r0"][t] + dt * v[0]
            P["y"][t] = P["r1"][t] + dt * v[1]
            P["z"][t] = P["r2"][t] + dt * v[2]
            P["r0"][t], P["r1"][t], P["r2"][t] = v


def advect(P, level, boxes, geom, dt, flags):
    advect_pass(P, level, boxes, geom, dt, 0, flags)
    advect_pass(P, level, boxes, geom, dt, 1, flags)


def sample(P, level, boxes, geom, comps, out, flags):
    """out[c, particle] for the valid particles of `level`; the other entries stay"""
    for b, t in _mine(P, level, len(boxes), flags):
        fab, abox, _ = boxes[b]
        clamped = None
        for c, comp in enumerate(comps):
            out[c, t], clamped = gather(fab, abox, geom, P["x"][t], P["y"][t], P["z"][t], comp)
        flags[0] += int(clamped.sum())


def _find_box(bl, grow, cell):
    for b, (vlo, vhi) in enumerate(bl):
        if all(vlo[d] - grow <= cell[d] <= vhi[d] + grow for d in range(3)):
            return b
    return -1


def locate(P, lev_min, lev_max, ngrow, level_boxes, geoms, flags):
    """Redistribute(lev_min, lev_max, ngrow); level_boxes[l] = [(vlo, vhi)], geoms[l] the geometry of level l"""
    g0 = geoms[0]
    periodic = [g0.lo_bc[d] == 0 and g0.hi_bc[d] == 0 for d in range(3)]
    for t in range(P["id"].shape[0]):
        if P["id"][t] <= 0 or P["level"][t] < lev_min:
            continue
        pos = [P["x"][t], P["y"][t], P["z"][t]]
        outside = False
        for d in range(3):
            plo, phi = g0.problo[d], g0.probhi[d]
            if periodic[d]:
                if abs(pos[d] - plo) < 1.0e3 * (phi - plo):
                    while pos[d] >= phi:
                        pos[d] = pos[d] - (phi - plo)
                    while pos[d] < plo:
                        pos[d] = pos[d] + (phi - plo)
                    if pos[d] == phi:
                        pos[d] = plo
            elif not (pos[d] >= plo and pos[d] < phi):
                outside = True
        P["x"][t], P["y"][t], P["z"][t] = pos
        if outside:
            P["id"][t] = -P["id"][t]
            continue
        for l in range(lev_max, lev_min - 1, -1):
            dxi = dxi_of(geoms[l])
            cell = [int(tr_floor((pos[d] - g0.problo[d]) * dxi[d])) for d in range(3)]
            b = _find_box(level_boxes[l], 0, cell)
            if b < 0 and l == lev_min and ngrow > 0:
                b = _find_box(level_boxes[l], ngrow, cell)
            if b >= 0:
                P["level"][t], P["grid"][t] = l, b
                break
        else:
            flags[1] += 1


def count(P, level, count_boxes, geom):
    """count_boxes: [(int32 array (nz, ny, nx), (alo, ahi))], incremented in place"""
    dxi = dxi_of(geom)
    for t in np.nonzero((P["id"] > 0) & (P["level"] == level))[0]:
        b = P["grid"][t]
        if b < 0 or b >= len(count_boxes):
            continue
        arr, (alo, ahi) = count_boxes[b]
        cell = [int(tr_floor((P[k][t] - geom.problo[d]) * dxi[d])) for d, k in enumerate("xyz")]
        if all(alo[d] <= cell[d] <= ahi[d] for d in range(3)):
            arr[cell[2] - alo[2], cell[1] - alo[1], cell[0] - alo[0]] += 1

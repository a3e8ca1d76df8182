"""numpy restatement of the boundary overrides of the state fill -- ambient_fill (Source/problems/ambient_fill.cpp:61-154) and
hse_fill (Source/problems/hse_fill.cpp) as ca_statefill calls them (Source/problems/Castro_bc_fill_nd.cpp:41-105) -- the CPU
reference of castro_amd_ext_bc_fill_fab.  Tests only.

Per-zone and per-column loops in the reference's order with Python floats (IEEE doubles), one accumulator, no vectorised
reordering: ambient_fill visits the zones with k outermost and i innermost, in place, so a zone that reads the domain's edge zone
of its line sees what the loop has made of that zone so far; hse_fill walks every ghost column outward from the domain.

A state is an array (8, nz, ny, nx) on the box [lo, hi].  geom: dx, domlo, domhi, lo_bc, hi_bc, coord; params: eos_gamma, abar;
ext: the fields of castro_amd_ext_bc."""
import numpy as np

URHO, UMX, UMY, UMZ, UEDEN, UEINT, UTEMP, UFS, NUM_STATE = 0, 1, 2, 3, 4, 5, 6, 7, 8
K_B, M_U = 1.3806488e-16, 1.660538921e-24           # castro_amd/csrc/hydro_device.h
INFLOW, OUTFLOW = 1, 2
EXT_HSE = 1
MAX_ITER, TOL = 250, 1.e-8                          # ext_bc_types.H


def _div(a, b):
    if b == 0.0:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))
    return a / b


def _amin(a, b):            # std::min / std::max: ties and NaNs resolve to the first argument
    return b if b < a else a


def _amax(a, b):
    return b if a < b else a


def e_of_T(T, xn, params):
    mu = _div(1.0, xn * (1.0 / params.abar))
    return _div(K_B * T, (params.eos_gamma - 1.0) * (mu * M_U))


def refusal(box, geom, ext, ncomp=NUM_STATE):
    """what castro_amd_ext_bc_fill_fab answers before it launches: None (it fills), "ok" (nothing to do), "unsupported", "arg" """
    lo, hi = box
    if ncomp != NUM_STATE:
        return "ok"
    if geom.coord != 0:
        return "unsupported"
    inflow = [geom.lo_bc[d] == INFLOW or geom.hi_bc[d] == INFLOW for d in range(3)]
    if sum(inflow) > 1:
        return "unsupported"
    if geom.hi_bc[2] == INFLOW and ext.hi_type[2] == EXT_HSE:
        return "unsupported"
    if any(hi[d] < geom.domlo[d] or lo[d] > geom.domhi[d] for d in range(3)):
        return "ok"
    for d, side in hse_faces(geom, ext):
        if ext.hse_interp_temp == 1 and geom.domhi[d] - geom.domlo[d] + 1 < 2:
            return "arg"
        nghost = geom.domlo[d] - lo[d] if side == 0 else hi[d] - geom.domhi[d]
        if nghost <= 0:
            continue
        ninside = (min(hi[d], geom.domhi[d]) - geom.domlo[d] + 1) if side == 0 else (geom.domhi[d] - max(lo[d], geom.domlo[d]) + 1)
        if ext.hse_interp_temp == 1 and ninside < 2:
            return "arg"
        if ext.hse_zero_vels != 1 and ext.hse_reflect_vels == 1 and ninside < nghost:
            return "arg"
    return None


def hse_faces(geom, ext):
    """(direction, side) of the faces with a hydrostatic fill: Inflow (EXT_DIR) and of type HSE"""
    out = []
    for d in range(3):
        if geom.lo_bc[d] == INFLOW and ext.lo_type[d] == EXT_HSE:
            out.append((d, 0))
        if geom.hi_bc[d] == INFLOW and ext.hi_type[d] == EXT_HSE:
            out.append((d, 1))
    return out


def ambient_fill(U, lo, hi, geom, ext):
    if ext.fill_ambient_bc != 1:
        return
    domlo, domhi = list(geom.domlo), list(geom.domhi)
    on = [ext.ambient_fill_dir in (d, -1) for d in range(3)]
    amb_lo = [on[d] and geom.lo_bc[d] == OUTFLOW for d in range(3)]
    amb_hi = [on[d] and geom.hi_bc[d] == OUTFLOW for d in range(3)]
    amb = [float(x) for x in ext.ambient_state]
    for k in range(lo[2], hi[2] + 1):
        for j in range(lo[1], hi[1] + 1):
            for i in range(lo[0], hi[0] + 1):
                z = (i, j, k)
                if not any((amb_lo[d] and z[d] < domlo[d]) or (amb_hi[d] and z[d] > domhi[d]) for d in range(3)):
                    continue
                at = (k - lo[2], j - lo[1], i - lo[0])
                for n in range(NUM_STATE):
                    U[(n,) + at] = amb[n]
                if ext.ambient_outflow_vel == 1:
                    # extrapolate the normal velocity only if it is outgoing: the chain x low, x high, y low, y high, z low, z high
                    for d in range(3):
                        if z[d] < domlo[d] or z[d] > domhi[d]:
                            break
                    s = list(z)
                    s[d] = domlo[d] if z[d] < domlo[d] else domhi[d]
                    edge = float(U[UMX + d, s[2] - lo[2], s[1] - lo[1], s[0] - lo[0]])
                    mom = [0.0, 0.0, 0.0]
                    mom[d] = _amin(0.0, edge) if z[d] < domlo[d] else _amax(0.0, edge)
                    for m in range(3):
                        U[(UMX + m,) + at] = mom[m]
                    # now make the energy consistent
                    U[(UEDEN,) + at] = amb[UEINT] + _div(0.5 * (mom[0] * mom[0] + mom[1] * mom[1] + mom[2] * mom[2]), amb[URHO])


def _hse_column(U, lo, hi, geom, params, ext, d, side, a, b):
    """one ghost column of face (d, side); (a, b): the indices along the two other directions.  Returns whether it converged"""
    step = 1 if side == 1 else -1
    dom = geom.domhi[d] if side == 1 else geom.domlo[d]
    end = hi[d] if side == 1 else lo[d]
    dx, grav, gm1 = float(geom.dx[d]), float(ext.const_grav), params.eos_gamma - 1.0

    def at(ii):
        ijk = [a, b]
        ijk.insert(d, ii)
        return (ijk[2] - lo[2], ijk[1] - lo[1], ijk[0] - lo[0])

    c0 = at(dom)
    dens_prev = float(U[(URHO,) + c0])
    temp_prev = float(U[(UTEMP,) + c0])
    X_zone = _div(float(U[(UFS,) + c0]), dens_prev)
    dens_base = dens_prev
    mom_base = [float(U[(UMX + m,) + c0]) for m in range(3)]
    pres_prev = gm1 * dens_prev * e_of_T(temp_prev, X_zone, params)
    all_converged = True
    ii = dom + step
    while (ii <= end) if side == 1 else (ii >= end):
        c = at(ii)
        dens_zone = dens_prev
        if ext.hse_interp_temp == 1:
            temp_zone = 2 * float(U[(UTEMP,) + at(ii - step)]) - float(U[(UTEMP,) + at(ii - 2 * step)])
        else:
            temp_zone = temp_prev
        e_zone = e_of_T(temp_zone, X_zone, params)
        converged = False
        for _ in range(MAX_ITER):
            if side == 1:
                p_want = pres_prev + dx * 0.5 * (dens_zone + dens_prev) * grav
            else:
                p_want = pres_prev - dx * 0.5 * (dens_zone + dens_prev) * grav
            pres_zone = gm1 * dens_zone * e_zone
            dpdr = _div(pres_zone, dens_zone)
            A = p_want - pres_zone
            if side == 1:
                drho = _div(A, dpdr - 0.5 * dx * grav)
            else:
                drho = _div(A, dpdr + 0.5 * dx * grav)
            dens_zone = _amax(0.9 * dens_zone, _amin(dens_zone + drho, 1.1 * dens_zone))
            if abs(drho) < TOL * dens_zone:
                converged = True
                break
        if not converged:
            all_converged = False
        if ext.hse_zero_vels == 1:
            mom = [0.0, 0.0, 0.0]
        elif ext.hse_reflect_vels == 1:
            off = ii - dom - 1 if side == 1 else dom - ii - 1
            cm = at(dom - off if side == 1 else dom + off)
            mom = [-dens_zone * _div(mom_base[m], dens_base) for m in range(3)]
            mom[d] = -dens_zone * _div(float(U[(UMX + d,) + cm]), float(U[(URHO,) + cm]))
        else:
            mom = [dens_zone * _div(mom_base[m], dens_base) for m in range(3)]
        pres_zone = gm1 * dens_zone * e_zone
        for m in range(3):
            U[(UMX + m,) + c] = mom[m]
        U[(URHO,) + c] = dens_zone
        U[(UEINT,) + c] = dens_zone * e_zone
        U[(UEDEN,) + c] = dens_zone * e_zone + _div(0.5 * (mom[0] * mom[0] + mom[1] * mom[1] + mom[2] * mom[2]), dens_zone)
        # hse_fill.cpp:963: the z-low face stores the temperature at the index of its ParallelFor, the first ghost zone
        U[(UTEMP,) + (at(dom - 1) if (d, side) == (2, 0) else c)] = temp_zone
        U[(UFS,) + c] = dens_zone * X_zone
        dens_prev, pres_prev = dens_zone, pres_zone
        ii += step
    return all_converged


def hse_fill(U, lo, hi, geom, params, ext):
    """returns the number of columns that left a Newton loop unconverged"""
    bad = 0
    for d, side in hse_faces(geom, ext):
        if (geom.domlo[d] - lo[d] if side == 0 else hi[d] - geom.domhi[d]) <= 0:
            continue
        t0, t1 = [e for e in range(3) if e != d]
        for b in range(lo[t1], hi[t1] + 1):
            for a in range(lo[t0], hi[t0] + 1):
                if not _hse_column(U, lo, hi, geom, params, ext, d, side, a, b):
                    bad += 1
    return bad


def ext_bc_fill(U, box, geom, params, ext):
    """ambient_fill, then hse_fill, in place on U (8, nz, ny, nx) of `box` = (lo, hi).  Returns the unconverged columns; raises
    ValueError where castro_amd_ext_bc_fill_fab returns an error code"""
    lo, hi = box
    r = refusal(box, geom, ext, U.shape[0])
    if r == "ok":
        return 0
    if r is not None:
        raise ValueError("ext_bc_fill: " + r)
    ambient_fill(U, lo, hi, geom, ext)
    return hse_fill(U, lo, hi, geom, params, ext)

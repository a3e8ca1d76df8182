"""numpy restatement of monopole gravity (tests only), written from the definitions in include/castro_hydro_amd.h -- operation by
operation, in that order, so that the bins of the sub-zones, the integration and the interpolation can be compared with the
kernels exactly -- and a CPU backend that adds the monopole methods of castro_amd.hydro.HipHydro to
tests/oracle_backend.OracleBackend.  The product never imports this file.

Binning.  The bins are integers and the volumes integer counts: both are compared exactly.  The mass of a bin is the exactly
rounded sum math.fsum of its terms vol_frac * rho.  Tolerance (derived, not tuned, as in tests/diag_ref.py): any order of N double
additions is within (N - 1) * 2**-53 * A of the exact sum to first order, A = fsum(|t_i|); the kernel's terms are the
restatement's bits in both builds (one multiplication, nothing to contract), so the bound of a bin is N_bin * 2**-52 * A_bin."""
import math

import numpy as np

from tests.oracle_backend import OracleBackend

URHO, UMX, UMY, UMZ, UEDEN = 0, 1, 2, 3, 4
NSRC = 7


def octant_factor(geom, mono):
    on = all(abs(mono.center[d] - geom.problo[d]) < 1.e-2 * geom.dx[d] for d in range(3))
    return 8.0 if on else 1.0


def vol_frac(geom, mono):
    fac = float(mono.drdxfac)
    return octant_factor(geom, mono) * (geom.dx[0] / fac) * (geom.dx[1] / fac) * (geom.dx[2] / fac)


def _axes(lo, shape, geom, mono, half):
    """problo + (index + half) * dx - center along x, y, z, broadcastable over (nz, ny, nx)"""
    nz, ny, nx = shape
    out = []
    for d, n in enumerate((nx, ny, nz)):
        v = geom.problo[d] + (np.arange(lo[d], lo[d] + n, dtype=np.float64) + half) * geom.dx[d] - mono.center[d]
        sh = [1, 1, 1]
        sh[2 - d] = n
        out.append(v.reshape(sh))
    return out


def radial_mass(boxes, geom, mono):
    """Gravity::compute_radial_mass.  boxes: [(rho (nz, ny, nx) of the valid zones, lo, mask (nz, ny, nx) uint8 or None)].
    Returns dict(mass=fsum per bin, count=int64 per bin, vol=count * vol_frac, A=fsum of |terms| per bin, dropped=sub-zones
    beyond the last bin or of zones whose centre lies beyond it, seq / vol_seq=the mass and the volume as the reference's single
    thread adds them: one accumulator per bin, the boxes in their order, the loop nest (k, j, i, kk, jj, ii) within a box --
    vol_seq adds vol_frac once per sub-zone and differs from count * vol_frac where a partial sum is inexact)."""
    n1d, f = mono.n1d, mono.drdxfac
    dr = geom.dx[0] / float(f)
    drinv = 1.0 / dr
    fac = float(f)
    frac = [geom.dx[d] / fac for d in range(3)]
    vf = vol_frac(geom, mono)
    idx_all, t_all, ord_all = [], [], []
    dropped = 0
    for nbox, (rho, lo, mask) in enumerate(boxes):
        rho = np.asarray(rho, dtype=np.float64)
        shape = rho.shape
        xc, yc, zc = _axes(lo, shape, geom, mono, 0.5)
        lo_i, lo_j, lo_k = _axes(lo, shape, geom, mono, 0.0)
        r = np.sqrt(xc * xc + yc * yc + zc * zc)
        index0 = np.floor(r * drinv).astype(np.int64)
        keep = (rho != 0.0)
        if mask is not None:
            keep &= (np.asarray(mask) != 0)
        dropped += int((keep & (index0 > n1d - 1)).sum()) * f ** 3
        keep &= index0 <= n1d - 1
        term = vf * rho
        zone = (np.arange(rho.size, dtype=np.int64).reshape(shape) + nbox * (1 << 32)) * f ** 3
        for kk in range(f):
            zz = lo_k + (float(kk) + 0.5) * frac[2]
            zzsq = zz * zz
            for jj in range(f):
                yy = lo_j + (float(jj) + 0.5) * frac[1]
                yysq = yy * yy
                for ii in range(f):
                    xx = lo_i + (float(ii) + 0.5) * frac[0]
                    xxsq = xx * xx
                    rr = np.sqrt(xxsq + yysq + zzsq)
                    index = np.floor(rr * drinv).astype(np.int64)
                    ok = keep & (index <= n1d - 1)
                    dropped += int((keep & ~ok).sum())
                    idx_all.append(index[ok])
                    t_all.append(np.broadcast_to(term, index.shape)[ok])
                    ord_all.append(zone[ok] + (kk * f + jj) * f + ii)
    idx = np.concatenate(idx_all) if idx_all else np.zeros(0, dtype=np.int64)
    t = np.concatenate(t_all) if t_all else np.zeros(0)
    count = np.bincount(idx, minlength=n1d).astype(np.int64)
    order = np.argsort(idx, kind="stable")
    ts = t[order]
    ends = np.cumsum(count)
    mass, A = np.zeros(n1d), np.zeros(n1d)
    for b in range(n1d):
        seg = ts[ends[b] - count[b]:ends[b]]
        if seg.size:
            mass[b] = math.fsum(seg.tolist())
            A[b] = math.fsum(np.abs(seg).tolist())
    seq, vol_seq = np.zeros(n1d), np.zeros(n1d)
    if idx.size:
        nest = np.argsort(np.concatenate(ord_all), kind="stable")
        for b, v in zip(idx[nest].tolist(), t[nest].tolist()):
            seq[b] += v
            vol_seq[b] += vf
    return dict(mass=mass, count=count, vol=count.astype(np.float64) * vf, A=A, dropped=dropped, seq=seq, vol_seq=vol_seq)


def mass_bounds(ref):
    """the tolerance of every bin's mass: N_bin * 2**-52 * A_bin (both builds)"""
    return ref["count"].astype(np.float64) * 2.0 ** -52 * ref["A"]


def radial_gravity(mass, vol, geom, mono):
    """the integration loop of make_radial_gravity (Gravity.cpp:3170-3274), no GR_GRAV"""
    n1d = mono.n1d
    dr = geom.dx[0] / float(mono.drdxfac)
    halfdr = 0.5 * dr
    Gconst, rmax = mono.Gconst, mono.max_radius_all_in_domain
    grav = np.zeros(n1d)
    mass_encl = 0.0
    vol_total_i = vol_outer_shell = vol_upper_shell = 0.0
    den_im1 = 0.0
    for i in range(n1d):
        m_i = float(mass[i])
        den_i = m_i
        if vol[i] > 0.0:
            den_i = den_i / float(vol[i])
        rlo = float(i) * dr
        rc = (float(i) + 0.5) * dr
        rhi = (float(i) + 1.0) * dr
        if i == 0:
            vol_outer_shell = (4.0 / 3.0 * math.pi) * rc * rc * rc
            vol_upper_shell = (4.0 / 3.0 * math.pi) * (rhi * rhi * rhi - rc * rc * rc)
            vol_total_i = vol_outer_shell + vol_upper_shell
            mass_encl = vol_outer_shell * m_i / vol_total_i
        else:
            vol_inner_shell = vol_upper_shell
            vol_total_im1 = vol_total_i
            vol_outer_shell = (4.0 / 3.0 * math.pi) * halfdr * (rc * rc + rlo * rc + rlo * rlo)
            vol_upper_shell = (4.0 / 3.0 * math.pi) * halfdr * (rc * rc + rhi * rc + rhi * rhi)
            vol_total_i = vol_outer_shell + vol_upper_shell
            if rc < rmax:
                mass_encl = mass_encl + (vol_inner_shell / vol_total_im1) * float(mass[i - 1]) + (vol_outer_shell / vol_total_i) * m_i
            else:
                mass_encl = mass_encl + vol_inner_shell * den_im1 + vol_outer_shell * den_i
        grav[i] = -Gconst * mass_encl / (rc * rc)
        den_im1 = den_i
    return grav


def interpolate(rg, geom, mono, grav, box, info=None):
    """interpolate_monopole_grav onto the whole of `grav` (3, nz, ny, nx) on `box`, in place; zones beyond the last bin keep
    what they hold.  Returns the bin of every zone; info (a dict): "clamp" = -1 / +1 where the minimum / maximum clamp of the
    quadratic branch changed the value, else 0."""
    n1d = mono.n1d
    rg = np.asarray(rg, dtype=np.float64)
    dr = geom.dx[0] / float(mono.drdxfac)
    shape = grav.shape[1:]
    loc = [a + np.zeros(shape) for a in _axes(box[0], shape, geom, mono, 0.5)]
    r = np.sqrt(loc[0] * loc[0] + loc[1] * loc[1] + loc[2] * loc[2])
    index = np.floor(r / dr).astype(np.int64)
    ic = np.clip(index, 1, n1d - 2)
    cen = (index.astype(np.float64) + 0.5) * dr
    xi = r - cen
    ghi, gmd, glo = rg[ic + 1], rg[ic], rg[ic - 1]
    quad = (ghi - 2.0 * gmd + glo) * xi * xi / (2.0 * dr * dr) + (ghi - glo) * xi / (2.0 * dr) + (-ghi + 26.e0 * gmd - glo) / 24.e0
    minvar, maxvar = np.minimum(gmd, np.minimum(glo, ghi)), np.maximum(gmd, np.maximum(glo, ghi))
    if info is not None:
        branch = (index > 0) & (index < n1d - 1)
        info["clamp"] = np.where(branch & (quad < minvar), -1, np.where(branch & (quad > maxvar), 1, 0))
    quad = np.minimum(np.maximum(quad, minvar), maxvar)
    first = rg[0] + ((rg[1] - rg[0]) / dr) * xi
    last = rg[n1d - 1] + ((rg[n1d - 1] - rg[n1d - 2]) / dr) * xi
    mag = np.where(index == 0, first, np.where(index == n1d - 1, last, quad))
    inside = index <= n1d - 1
    with np.errstate(all="ignore"):
        for n in range(3):
            grav[n][inside] = (mag * (loc[n] / r))[inside]
    return index


def _sl(box, lo, hi, off=(0, 0, 0)):
    return tuple(slice(lo[a] - box[0][a] + off[a], hi[a] - box[0][a] + 1 + off[a]) for a in (2, 1, 0))


def old_gravity_source(U, box, gold, gbox, lo, hi, gtype, dt):
    """Castro::construct_old_gravity_source with a per-zone vector: the NSRC source components on [lo, hi]"""
    u = np.asarray(U)[(slice(None),) + _sl(box, lo, hi)]
    g = np.asarray(gold)[(slice(None),) + _sl(gbox, lo, hi)]
    rho = u[URHO]
    rhoInv = 1.0 / rho
    snew = [u[n].copy() for n in range(8)]
    old_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoInv
    src = np.zeros((NSRC,) + rho.shape)
    Sr = []
    for n in range(3):
        Sr.append(rho * g[n])
        src[UMX + n] = Sr[n]
        snew[UMX + n] = snew[UMX + n] + dt * src[UMX + n]
    if gtype == 3:
        new_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoInv
        SrE = new_ke - old_ke
    else:
        SrE = (u[UMX] * Sr[0] + u[UMY] * Sr[1] + u[UMZ] * Sr[2]) * rhoInv
    src[UEDEN] = SrE
    return src


def new_gravity_source(UO, obox, UN, nbox, M, mboxes, gold, gnew, gbox, lo, hi, gtype, dt, dx):
    """Castro::construct_new_gravity_source with per-zone vectors gold / gnew (one ghost zone around [lo, hi] for type 4)"""
    uo = np.asarray(UO)[(slice(None),) + _sl(obox, lo, hi)]
    un = np.asarray(UN)[(slice(None),) + _sl(nbox, lo, hi)]
    gold, gnew = np.asarray(gold), np.asarray(gnew)
    go = gold[(slice(None),) + _sl(gbox, lo, hi)]
    gn = gnew[(slice(None),) + _sl(gbox, lo, hi)]
    vol = dx[0] * dx[1] * dx[2]
    hdtInv = 0.5 / dt
    rhoo, rhooinv = uo[URHO], 1.0 / uo[URHO]
    rhon, rhoninv = un[URHO], 1.0 / un[URHO]
    snew = [un[n].copy() for n in range(8)]
    old_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoninv
    vold = [uo[UMX + n] * rhooinv for n in range(3)]
    Sr_old = [rhoo * go[n] for n in range(3)]
    SrE_old = vold[0] * Sr_old[0] + vold[1] * Sr_old[1] + vold[2] * Sr_old[2]
    vnew = [snew[UMX + n] * rhoninv for n in range(3)]
    Sr_new = [rhon * gn[n] for n in range(3)]
    SrE_new = vnew[0] * Sr_new[0] + vnew[1] * Sr_new[1] + vnew[2] * Sr_new[2]
    src = np.zeros((NSRC,) + rhoo.shape)
    for n in range(3):
        src[UMX + n] = 0.5 * (Sr_new[n] - Sr_old[n])
        snew[UMX + n] = snew[UMX + n] + dt * src[UMX + n]
    if gtype == 1:
        SrEcorr = 0.5 * (SrE_new - SrE_old)
    elif gtype == 2:
        vnew = [snew[UMX + n] * rhoninv for n in range(3)]
        SrE_new = vnew[0] * Sr_new[0] + vnew[1] * Sr_new[1] + vnew[2] * Sr_new[2]
        SrEcorr = 0.5 * (SrE_new - SrE_old)
    elif gtype == 3:
        new_ke = 0.5 * (snew[UMX] * snew[UMX] + snew[UMY] * snew[UMY] + snew[UMZ] * snew[UMZ]) * rhoninv
        SrEcorr = new_ke - old_ke
    else:
        g = [0.5 * (gn[n] + go[n]) for n in range(3)]
        edge = []
        for n in range(3):
            for side in (-1, 1):
                off = [0, 0, 0]
                off[n] = side
                s = _sl(gbox, lo, hi, off)
                edge.append(0.5 * (g[n] + 0.5 * (gnew[n][s] + gold[n][s])))
        fl = []
        for n in range(3):
            off = [0, 0, 0]
            off[n] = 1
            m = np.asarray(M[n])[0]
            fl += [m[_sl(mboxes[n], lo, hi)], m[_sl(mboxes[n], lo, hi, off)]]
        SrEcorr = -SrE_old + hdtInv * (fl[0] * edge[0] * dx[0] + fl[1] * edge[1] * dx[0] + fl[2] * edge[2] * dx[1] +
                                       fl[3] * edge[3] * dx[1] + fl[4] * edge[4] * dx[2] + fl[5] * edge[5] * dx[2]) / vol
    src[UEDEN] = SrEcorr
    return src


class MonopoleOracleBackend(OracleBackend):
    """OracleBackend + the monopole methods, in numpy.  ulps: the radial masses are moved by that many units in the last place
    in front of the sum over the ranks (the sensitivity probe of the driver test)."""

    def __init__(self, nthreads=1, ulps=0):
        super().__init__(nthreads)
        self.ulps = int(ulps)

    @staticmethod
    def make_diag_boxes(specs):
        return list(specs), len(specs)

    def radial_mass_mf(self, boxes, geom, mono, out, stream=None):
        specs, _ = boxes
        rb = []
        for lo, hi, (S, sbox), mask in specs:
            rb.append((S.numpy()[(URHO,) + _sl(sbox, lo, hi)], lo, None if mask is None else mask.numpy()))
        ref = radial_mass(rb, geom, mono)
        mass = ref["mass"]
        for _ in range(abs(self.ulps)):
            mass = np.nextafter(mass, np.inf if self.ulps > 0 else -np.inf)
        o = out.numpy()
        o[:mono.n1d] = mass
        o[mono.n1d:] = ref["vol"]

    def radial_gravity(self, mono, geom, mass_vol, radial_grav, stream=None):
        mv = mass_vol.numpy()
        radial_grav.numpy()[:] = radial_gravity(mv[:mono.n1d], mv[mono.n1d:], geom, mono)

    def monopole_grav(self, radial_grav, mono, geom, grav, grav_box, stream=None):
        interpolate(radial_grav.numpy(), geom, mono, grav.numpy(), grav_box)

    def old_gravity_source_gfab(self, state, box, source, src_box, lo, hi, grav_old, grav_box, grav_source_type, dt, stream=None):
        s = source.numpy()[(slice(0, NSRC),) + _sl(src_box, lo, hi)]
        s += old_gravity_source(state.numpy(), box, grav_old.numpy(), grav_box, lo, hi, int(grav_source_type), float(dt))

    def new_gravity_source_gfab(self, state_old, old_box, state_new, new_box, source, src_box, mass_fluxes, flux_boxes, lo, hi,
                                grav_old, grav_new, grav_box, grav_source_type, dt, geom, stream=None):
        s = source.numpy()[(slice(0, NSRC),) + _sl(src_box, lo, hi)]
        s += new_gravity_source(state_old.numpy(), old_box, state_new.numpy(), new_box, [m.numpy() for m in mass_fluxes], flux_boxes,
                                grav_old.numpy(), grav_new.numpy(), grav_box, lo, hi, int(grav_source_type), float(dt),
                                [geom.dx[d] for d in range(3)])


# ---- the dust-collapse driver case shared by the CPU and the GPU tests ----------------------------------------------------------
# Exec/gravity_tests/DustCollapse/inputs_3d_monopole_regtest on 16^3 zones: the octant, Symmetry below and outflow above
DUST_N, DUST_STEPS, DUST_DRDXFAC = (16, 16, 16), 3, 4
DUST_GEOM = dict(prob_lo=(0., 0., 0.), prob_hi=(7.5e8, 7.5e8, 7.5e8), lo_bc=(3, 3, 3), hi_bc=(2, 2, 2))
DUST_PROB = dict(rho_0=1.e9, r_0=6.5e8, p_0=1.e15, rho_ambient=1.0e-5, smooth_delta=4.e6, nsub=5)
DUST_PARAMS = dict(eos_gamma=1.66666, small_dens=1.e-6, small_temp=1.e-3, cfl=0.5, init_shrink=0.1, change_max=1.05)


def dust_collapse_run(hydro, params, comm=None, do_grav=True, steps=DUST_STEPS, **kw):
    """(driver, [dt of every step]) of the dust-collapse case on `hydro`"""
    import castro_amd
    c = castro_amd.Castro(DUST_N, params=params, hydro=hydro, comm=comm, do_grav=do_grav, gravity_type="monopole",
                          drdxfac=DUST_DRDXFAC, **DUST_GEOM, **kw)
    c.center = (0.0, 0.0, 0.0)
    c.initData("dust_collapse", **DUST_PROB)
    return c, [c.step() for _ in range(steps)]


def field_deviation(a, b):
    """max |a - b| of every state component over the largest magnitude of the field in b (the three momenta are one field)"""
    a, b = np.asarray(a), np.asarray(b)
    scale = [np.abs(b[n]).max() for n in range(b.shape[0])]
    mom = max(scale[UMX], scale[UMY], scale[UMZ])
    for n in (UMX, UMY, UMZ):
        scale[n] = mom
    return np.array([np.abs(a[n] - b[n]).max() / max(scale[n], 1e-300) for n in range(b.shape[0])])


def dust_sensitivity(oracle):
    """(reference driver, its dts, s): the run on MonopoleOracleBackend, and the deviation per field that a second run shows
    whose radial masses differ by one ulp per bin -- what a different order of the bin sums can do to the result (the
    convention of tools/fuzz_contract.py); the tolerance of a comparison is max(1e-10, 100 * s) of the field's max"""
    ref, dts = dust_collapse_run(MonopoleOracleBackend(), oracle.default_params(**DUST_PARAMS))
    ulp, _ = dust_collapse_run(MonopoleOracleBackend(ulps=1), oracle.default_params(**DUST_PARAMS))
    s = field_deviation(ulp.S_new().numpy(), ref.S_new().numpy())
    return ref, dts, s

"""numpy restatement of the thermal-diffusion term and of its time-step limit (tests only), written from the definition in
include/castro_hydro_amd.h -- operation by operation, in that order, so that the `exact` build can be compared bit for bit --
and a CPU backend that adds the two diffusion methods of castro_amd.hydro.HipHydro to tests/oracle_backend.OracleBackend.
The product never imports this file."""
import numpy as np

from tests.oracle_backend import OracleBackend

URHO, UEDEN, UEINT, UTEMP, UFS = 0, 4, 5, 6, 7
K_B, M_U = 1.3806488e-16, 1.660538921e-24


def cond_cc(rho, diff):
    """cell-centred conductivity: 0 at or below the cutoff, ramped up to cutoff_hi, times the scale factor"""
    cut, cut_hi = diff.diffuse_cutoff_density, diff.diffuse_cutoff_density_hi
    with np.errstate(all="ignore"):
        on = rho > cut
        ramp = on & (rho < cut_hi)
        cond = np.where(on, diff.const_conductivity, 0.0)
        mult = (rho - cut) / (cut_hi - cut)
        cond = np.where(ramp, cond * mult, cond)
    return diff.diffuse_cond_scale_fac * cond


def diffusion_term(U, box, lo, hi, geom, diff):
    """(DiffTerm, A) on [lo, hi] from the state U (8, nz, ny, nx) on `box`, which holds one ghost zone around [lo, hi].
    A: the sum of the absolute face contributions, dhx * (|b dT| of the two x faces) + ... (the scale of the round-off)."""
    blo = box[0]
    T = np.asarray(U[UTEMP])
    kc = cond_cc(np.asarray(U[URHO]), diff)

    def sl(off):
        return tuple(slice(lo[2 - a] - blo[2 - a] + off[2 - a], hi[2 - a] - blo[2 - a] + 1 + off[2 - a]) for a in range(3))

    c = sl((0, 0, 0))
    f, fa = [], []
    for d in range(3):
        op, om = [0, 0, 0], [0, 0, 0]
        op[d], om[d] = 1, -1
        p, m = sl(op), sl(om)
        with np.errstate(all="ignore"):
            bhi = 0.5 * (kc[p] + kc[c])
            bl = 0.5 * (kc[c] + kc[m])
            fhi = bhi * (T[p] - T[c])
            flo = bl * (T[c] - T[m])
        idx = np.arange(lo[d], hi[d] + 1)
        shape = [1, 1, 1]
        shape[2 - d] = idx.size
        idx = idx.reshape(shape)
        if geom.hi_bc[d] != 0:                     # a physical boundary: zero flux whatever the ghost zone holds
            fhi = np.where(idx == geom.domhi[d], 0.0, fhi)
        if geom.lo_bc[d] != 0:
            flo = np.where(idx == geom.domlo[d], 0.0, flo)
        f.append(fhi - flo)
        fa.append(np.abs(fhi) + np.abs(flo))
    dh = [1.0 / (geom.dx[d] * geom.dx[d]) for d in range(3)]
    D = dh[0] * f[0] + dh[1] * f[1] + dh[2] * f[2]
    A = dh[0] * fa[0] + dh[1] * fa[1] + dh[2] * fa[2]
    return D, A


def supported(geom):
    """Inflow on a low face and Symmetry on a high face are Dirichlet in the reference: not restated"""
    return geom.coord == 0 and all(geom.lo_bc[d] != 1 and geom.hi_bc[d] != 3 for d in range(3))


def estdt_temp_diffusion(U, box, lo, hi, geom, params, diff, max_dt):
    """min over [lo, hi] of 0.5 dx_d^2 / D, D = conductivity / (rho c_v) (raw conductivity); max_dt / cfl at or below the cutoff"""
    blo = box[0]
    sl = tuple(slice(lo[2 - a] - blo[2 - a], hi[2 - a] - blo[2 - a] + 1) for a in range(3))
    rho = np.asarray(U[URHO])[sl]
    rX = np.asarray(U[UFS])[sl]
    with np.errstate(all="ignore"):
        rho_inv = 1.0 / rho
        xn = rX * rho_inv
        mu = 1.0 / (xn * (1.0 / params.abar))
        cv = K_B / ((params.eos_gamma - 1.0) * (mu * M_U))
        Dc = diff.const_conductivity * rho_inv / cv
        dts = [0.5 * geom.dx[d] * geom.dx[d] / Dc for d in range(3)]
        v = np.minimum(np.minimum(dts[0], dts[1]), dts[2])
    v = np.where(rho > diff.diffuse_cutoff_density, v, max_dt / params.cfl)
    return float(np.nanmin(v))


# ---- inputs and restatements of the unit tests -------------------------------------------------------------------------------
def grow(lo, hi, g):
    return tuple(x - g for x in lo), tuple(x + g for x in hi)


def shape_of(box):
    """(nz, ny, nx) of an array on `box`"""
    return tuple(box[1][a] - box[0][a] + 1 for a in (2, 1, 0))


def region(box, lo, hi):
    """the slices (z, y, x) of [lo, hi] in an array on `box`"""
    return tuple(slice(lo[a] - box[0][a], hi[a] - box[0][a] + 1) for a in (2, 1, 0))


def random_state(rng, shape):
    """the recipe of the unit case: every component uniform in (0.5, 3.5), so that with a cutoff of 1 and a cutoff_hi of 2.5
    a sixth of the densities lies at or below the cutoff, half on the ramp and a third above it; T uniform in (1, 2)"""
    U = rng.uniform(0.5, 3.5, size=(8,) + tuple(shape))
    U[UTEMP] = rng.uniform(1.0, 2.0, size=tuple(shape))
    return U


def fill_ghosts(U, lo, hi, g, geom):
    """what the ghost zones of a FAB on grow([lo, hi], g) hold in front of the term: the periodic image where the box spans a
    periodic direction, NaN behind a physical face (the operator must not use it), and the values U came with (finite: the
    neighbour box's data) wherever the edge of the box is interior to the domain"""
    for d in range(3):
        ax = 3 - d
        n = hi[d] - lo[d] + 1
        at_lo, at_hi = lo[d] == geom.domlo[d], hi[d] == geom.domhi[d]
        if geom.lo_bc[d] == 0 and geom.hi_bc[d] == 0:
            if at_lo and at_hi:
                U[...] = np.take(U, g + (np.arange(-g, n + g) % n), axis=ax)
            continue
        idx = [slice(None)] * 4
        if at_lo and geom.lo_bc[d] != 0:
            idx[ax] = slice(0, g)
            U[tuple(idx)] = np.nan
        if at_hi and geom.hi_bc[d] != 0:
            idx[ax] = slice(n + g, n + 2 * g)
            U[tuple(idx)] = np.nan
    return U


def ghosted_state(rng, lo, hi, g, geom):
    """(U, box): a random state (random_state) on grow([lo, hi], g) with the ghost zones of fill_ghosts"""
    box = grow(lo, hi, g)
    return fill_ghosts(random_state(rng, shape_of(box)), lo, hi, g, geom), box


def source_stage(stage, S_old, old_box, S_new, new_box, src_box, src_ncomp, lo, hi, geom, diff, dt):
    """castro_amd_sources_mf_ex without gravity, rotation and clean_state, for one box: (source, S_new after the stage, A).
      stage 0: source(UEDEN, UEINT) = 0 + 1.0 * D(S_old);                        S_new = S_old + dt * source on [lo, hi]
      stage 1: source(UEDEN, UEINT) = (0 + 0.5 * D(S_new)) + (-0.5) * D(S_old);  S_new += dt * source
    every other component and every zone of the source FAB outside [lo, hi] is zero; A: the |m|-weighted sum of the terms' A"""
    Do, Ao = diffusion_term(S_old, old_box, lo, hi, geom, diff)
    nv = (slice(None),) + region(new_box, lo, hi)
    if stage == 0:
        term = 0.0 + 1.0 * Do
        A = Ao
        base = S_old[(slice(None),) + region(old_box, lo, hi)]
    else:
        Dn, An = diffusion_term(S_new, new_box, lo, hi, geom, diff)
        term = (0.0 + 0.5 * Dn) + (-0.5) * Do
        A = 0.5 * An + 0.5 * Ao
        base = S_new[nv]
    src = np.zeros((src_ncomp,) + shape_of(src_box))
    sv = region(src_box, lo, hi)
    src[UEDEN][sv] = term
    src[UEINT][sv] = term
    upd = base.copy()
    upd[:7] = base[:7] + dt * src[(slice(0, 7),) + sv]
    out = S_new.copy()
    out[nv] = upd
    return src, out, A


class DiffusionOracleBackend(OracleBackend):
    """OracleBackend + the diffusion methods, in numpy"""

    def temp_diffusion(self, state, box, source, src_box, lo, hi, diffusion, geom, mult=1.0, diff_term=None, diff_term_box=None,
                       stream=None):
        assert supported(geom)
        D, _ = diffusion_term(state.numpy(), box, lo, hi, geom, diffusion)
        if source is not None:
            s = source.numpy()
            sl = self._slices(src_box, lo, hi)[1:]
            for n in (UEDEN, UEINT):
                s[n][sl] = s[n][sl] + mult * D
        if diff_term is not None:
            diff_term.numpy()[0][self._slices(diff_term_box, lo, hi)[1:]] = D

    def estdt_temp_diffusion(self, state, box, lo, hi, geom, params, diffusion, max_dt, out, stream=None):
        e = estdt_temp_diffusion(state.numpy(), box, lo, hi, geom, params, diffusion, max_dt)
        out[0] = min(out[0].item(), e)

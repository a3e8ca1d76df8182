"""castro.update_sources_after_reflux (CastroAmr(update_sources_after_reflux=True)): the CPU backend of the one new driver call
and what the CPU and the GPU tests share -- the geometry, the initial data, and the consistency measure of the stored new-time
source.  The product never imports this file.

Geometry: the smallest with every case.  A 16 x 8 x 8 coarse domain of cubic zones in two 8^3 boxes, periodic in x; the fine level
(ratio 2) is two 8^3 boxes over the coarse zones x = 8..11 and x = 12..15, y, z = 2..5.  They share the face x = 12 (fine-fine: it
receives nothing), the first has its low x face on the seam of the two coarse boxes (its outside neighbours live in the other
coarse box), the second touches the periodic boundary (its high x register wraps to the coarse face x = 0, which is also the
face x = 16 of the second coarse box); the y and z faces are coarse-fine faces of the other four orientations; no box starts
at 0 in every direction."""
import numpy as np
import torch

from tests.oracle_backend import OracleBackend

N_CELL, PROB_HI, BASE_GRID = (16, 8, 8), (2.0, 1.0, 1.0), (2, 1, 1)
FINE = [((8, 2, 2), (11, 5, 5)), ((12, 2, 2), (15, 5, 5))]
FINER = [((18, 6, 6), (21, 9, 9))]             # a level-2 box inside the first level-1 box (level-1 zones 16..23, 4..11)
PERIODIC_X = dict(lo_bc=(0, 2, 2), hi_bc=(0, 2, 2))
OPEN = dict(lo_bc=(2, 2, 2), hi_bc=(2, 2, 2))
NSRC = 7


class RegToFlux:
    """the register-to-flux operation in numpy: flux += reg on the faces [lo, hi], mass_flux = flux(URHO) there"""

    def fluxreg_to_flux(self, flux, flux_box, reg, reg_box, mass_flux, mass_box, lo, hi, ncomp, stream=None):
        f = flux.numpy()[OracleBackend._slices(flux_box, lo, hi)]
        f[:ncomp] += reg.numpy()[OracleBackend._slices(reg_box, lo, hi)][:ncomp]
        if mass_flux is not None:
            mass_flux.numpy()[OracleBackend._slices(mass_box, lo, hi)][0] = f[0]


class RefluxOracleBackend(RegToFlux, OracleBackend):
    """OracleBackend + the register-to-flux operation: everything else the re-evaluation needs -- the removal of the stored source
    as saxpy + clean_state, the new-source calls -- is there"""


def full_backend():
    """the same on the backend that carries monopole gravity, the point mass and the sponge in numpy"""
    from tests.pointmass_ref import PointMassOracleBackend

    class RefluxFullOracleBackend(RegToFlux, PointMassOracleBackend):
        pass
    return RefluxFullOracleBackend


def blob_state(params, n, prob_hi=PROB_HI, center=(1.02, 0.52, 0.27), width=0.17, rho_blob=6.0, vel=(1.1, 0.45, 0.6), p0=1.0):
    """A dense Gaussian blob (rho = 1 + rho_blob exp(-r^2 / width^2)) in pressure equilibrium, the whole gas moving with `vel`:
    the blob sits on the low x and the low z faces of the fine region and crosses them.  (NUM_STATE, nz, ny, nx) on n zones."""
    from castro_amd import _lib
    ax = [(np.arange(n[d]) + 0.5) * (prob_hi[d] / n[d]) - center[d] for d in range(3)]
    X, Y, Z = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
    rho = 1.0 + rho_blob * np.exp(-(X * X + Y * Y + Z * Z) / (width * width))
    U = np.zeros((8,) + rho.shape)
    U[0] = rho
    for k in range(3):
        U[1 + k] = rho * vel[k]
    U[5] = p0 / (params.eos_gamma - 1.0)
    U[4] = U[5] + 0.5 * rho * sum(v * v for v in vel)
    U[6] = U[5] / (rho * _lib.gamma_law_cv(params))
    U[7] = rho
    return U


def make_amr(make_hydro, params, option, patches=None, base_grid=BASE_GRID, bc=PERIODIC_X, **kw):
    import castro_amd
    return castro_amd.CastroAmr(N_CELL, patches=[FINE] if patches is None else patches, prob_hi=PROB_HI, params=params,
                                make_hydro=make_hydro, base_grid=base_grid, update_sources_after_reflux=option, **dict(bc, **kw))


def init_state(a, state_of=blob_state, **kw):
    """CastroAmr.initData with a host function of (params, zones of the level): every level from the function, averaged down"""
    a.invalidate_estimates()
    for l, lev in enumerate(a.lev):
        U = None
        for b in lev.mine:
            if U is None:
                U = state_of(a.params, tuple((2 ** l) * x for x in N_CELL), **kw)
            b.set_state(U)
    for l in range(len(a.lev) - 1, 0, -1):
        a.avgDown(l)
    a.time, a.nstep = 0.0, 0


def covered(a, l):
    """bool [nz, ny, nx] over the domain of level l: the zones level l + 1 covers"""
    n = tuple((2 ** l) * x for x in N_CELL)
    c = np.zeros(n[::-1], dtype=bool)
    if l + 1 < len(a.lev):
        for f in a.lev[l + 1].boxes:
            (lo, hi) = f.pbox
            c[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    return c


def boundary_zones(a, l):
    """bool [nz, ny, nx] over the domain of level l: the uncovered zones with a face on the boundary of level l + 1"""
    c = covered(a, l)
    near = np.zeros_like(c)
    for d in range(3):
        ax = 2 - d
        for s in (-1, 1):
            if a.periodic[d]:
                near |= np.roll(c, s, axis=ax)
            else:
                sh = np.zeros_like(c)
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                src[ax], dst[ax] = (slice(0, -1), slice(1, None)) if s == 1 else (slice(1, None), slice(0, -1))
                sh[tuple(dst)] = c[tuple(src)]
                near |= sh
    return near & ~c


def new_source_from(b, U, dt):
    """the new-time source of box b by the separate backend calls, from (S_old, U, mass fluxes, gravity FABs) as they stand"""
    h = b.hydro
    src = torch.zeros_like(b.new_source)
    S, g, lo, hi, sbx = b.S_old_b, b.gbox, b.lo, b.hi, b.bx
    if b.grav_fab:
        h.new_gravity_source_gfab(S, g, U, g, src, sbx, b.mass_fluxes, b.flux_boxes, lo, hi, b.grav_old, b.grav_new, b.gravbox,
                                  b.grav_source_type, dt, b.geom)
    elif b.do_grav:
        h.new_gravity_source(S, g, U, g, src, sbx, b.mass_fluxes, b.flux_boxes, lo, hi, b.grav, b.grav_source_type, dt, b.geom)
    if b.rotation is not None:
        h.new_rotation_source(S, g, U, g, src, sbx, b.mass_fluxes, b.flux_boxes, lo, hi, b.rotation, b.geom, dt)
    if b.sponge is not None:
        h.new_sponge_source(U, g, src, sbx, lo, hi, b._sponge_params(), b.geom, b.params, dt)
    return src


def corrector_mismatch(a, l, zones=None):
    """max |stored new_source - new-time source evaluated from (S_old, S_new - dt x new_source, mass fluxes, gravity)| over
    `zones` (bool over the level's domain; default: every zone of the level's boxes), over max |new_source| of the level"""
    lev = a.lev[l]
    dt = lev.lastDt
    num = den = 0.0
    for b in lev.mine:
        U = b.S_new_b.clone()
        b.hydro.saxpy(U, b.gbox, -dt, b.new_source, b.bx, NSRC, b.lo, b.hi)
        diff = (new_source_from(b, U, dt) - b.new_source).abs().cpu().numpy()
        if zones is not None:
            diff = diff[:, zones[b.lo[2]:b.hi[2] + 1, b.lo[1]:b.hi[1] + 1, b.lo[0]:b.hi[0] + 1]]
        num = max(num, float(diff.max()) if diff.size else 0.0)
        den = max(den, float(b.new_source.abs().max()))
    return num / den


def level_arrays(a, name="S_new"):
    """[[numpy array per box] per level] of S_new (valid zones) or new_source"""
    get = (lambda b: b.S_new()) if name == "S_new" else (lambda b: getattr(b, name))
    return [[get(b).cpu().numpy().copy() for b in lev.mine] for lev in a.lev]

"""numpy restatement of the sponge (castro.do_sponge, Source/sources/Castro_sponge.cpp:55-249) -- the CPU reference of
castro_amd_new_sponge_source_fab and of the sponge term of the one-pass source kernel, with the operation order of the
reference: 1 / rho once, (x - lo) / delta, (U - rho v_t) * fac / dt left to right.  Tests only.

apply_sponge() returns the source of every zone of [lo, hi] and, with info={}, the sponge factor and the mask of the zones whose
factor went through a cos (the only place where the device and glibc may differ)."""
import numpy as np

from tests.monopole_ref import MonopoleOracleBackend, _sl

URHO, UMX, UMY, UMZ, UEDEN, UEINT, UTEMP, UFS, NSRC = 0, 1, 2, 3, 4, 5, 6, 7, 7
# CODATA-2010 cgs constants of the gamma-law restatement (castro_amd/csrc/hydro_device.h)
K_B, M_U = 1.3806488e-16, 1.660538921e-24


def pressure_rt(rho, T, xn, params):
    """eos(eos_input_rt) of the gamma-law gas as the kernels write it: e = k T / ((gamma - 1) (mu m_u)), p = (gamma - 1) rho e"""
    mu = 1.0 / (xn * (1.0 / params.abar))
    e = K_B * T / ((params.eos_gamma - 1.0) * (mu * M_U))
    return (params.eos_gamma - 1.0) * rho * e


def _ramp(sp, x, lo, delta):
    with np.errstate(all="ignore"):
        return sp.lower_factor + 0.5 * (sp.upper_factor - sp.lower_factor) * (1.0 - np.cos(np.pi * (x - lo) / delta))


def sponge_factor(sp, rad, rho, p, info=None):
    """the sponge factor of zones at radius rad with density rho and pressure p, and which ramps were evaluated"""
    f = np.zeros_like(rho)
    cosm = np.zeros(rho.shape, dtype=bool)
    region = {}
    if sp.lower_radius >= 0.0 and sp.upper_radius > sp.lower_radius:
        below, on = rad < sp.lower_radius, (rad >= sp.lower_radius) & (rad <= sp.upper_radius)
        f = np.where(below, sp.lower_factor, np.where(on, _ramp(sp, rad, sp.lower_radius, sp.upper_radius - sp.lower_radius),
                                                      sp.upper_factor))
        cosm = on
        region["radius"] = (below, on, ~(below | on))
    if sp.upper_density > 0.0 and sp.lower_density > 0.0:
        above, on = rho > sp.upper_density, (rho <= sp.upper_density) & (rho >= sp.lower_density)
        f = np.where(above, sp.lower_factor, np.where(on, _ramp(sp, rho, sp.upper_density, sp.lower_density - sp.upper_density),
                                                      sp.upper_factor))
        cosm = on
        region["density"] = (~(above | on), on, above)
    if sp.upper_pressure > 0.0 and sp.lower_pressure >= 0.0:
        above, on = p > sp.upper_pressure, (p <= sp.upper_pressure) & (p >= sp.lower_pressure)
        f = np.where(above, sp.lower_factor, np.where(on, _ramp(sp, p, sp.upper_pressure, sp.lower_pressure - sp.upper_pressure),
                                                      sp.upper_factor))
        cosm = on
        region["pressure"] = (~(above | on), on, above)
    if info is not None:
        info["factor"], info["cos"], info["region"] = f, cosm, region
    return f


def radius(sp, geom, lo, hi):
    """|problo + (i + 1/2) dx - center| of the zones of [lo, hi], (nz, ny, nx)"""
    r = [geom.problo[d] + (np.arange(lo[d], hi[d] + 1).astype(np.float64) + 0.5) * geom.dx[d] - sp.center[d] for d in range(3)]
    X, Y, Z = r[0][None, None, :], r[1][None, :, None], r[2][:, None, None]
    return np.sqrt(X * X + Y * Y + Z * Z)


def apply_sponge(U, box, lo, hi, sp, geom, params, dt, info=None):
    """Castro::apply_sponge on [lo, hi] of the state U (8 components on `box`): the NSRC source components, zero except
    UMX..UMZ and UEDEN"""
    u = np.asarray(U)[(slice(None),) + _sl(box, lo, hi)]
    rho = u[URHO]
    rhoInv = 1.0 / rho
    alpha = dt / sp.timescale if sp.timescale > 0.0 else 0.0
    p = pressure_rt(rho, u[UTEMP], u[UFS] * rhoInv, params)
    f = sponge_factor(sp, radius(sp, geom, lo, hi), rho, p, info)
    if sp.implicit == 1:
        fac = -(1.0 - 1.0 / (1.0 + alpha * f))
    else:
        fac = -alpha * f
    src = np.zeros((NSRC,) + rho.shape)
    SrE = np.zeros_like(rho)
    for n in range(3):
        Sr = (u[UMX + n] - rho * sp.target_velocity[n]) * fac / dt
        src[UMX + n] = Sr
        SrE = SrE + u[UMX + n] * rhoInv * Sr
    src[UEDEN] = SrE
    if info is not None:
        info["alpha"], info["pressure"] = alpha, p
    return src


def cos_bound(U, box, lo, hi, sp, src, dt):
    """the permitted |device - glibc| of the momentum sources of a ramp zone, per momentum component (3, nz, ny, nx):
    8 * 2^-52 * (|U_m - rho v_t| * alpha * |upper_factor - lower_factor| / dt + |Sr|) -- a 4-ulp cos through
    0.5 (uf - lf) (1 - cos) and |dfac/df| <= alpha, doubled"""
    u = np.asarray(U)[(slice(None),) + _sl(box, lo, hi)]
    alpha = dt / sp.timescale
    return np.stack([8.0 * 2.0 ** -52 * (np.abs(u[UMX + n] - u[URHO] * sp.target_velocity[n]) * alpha
                                         * abs(sp.upper_factor - sp.lower_factor) / dt + np.abs(src[UMX + n])) for n in range(3)])


class SpongeOracleBackend(MonopoleOracleBackend):
    """MonopoleOracleBackend + new_sponge_source: the CPU drivers take the separate-call path with it"""

    def new_sponge_source(self, state_new, new_box, source, src_box, lo, hi, sponge, geom, params, dt, stream=None):
        s = source.numpy()[(slice(0, NSRC),) + _sl(src_box, lo, hi)]
        add = apply_sponge(state_new.numpy(), new_box, lo, hi, sponge, geom, params, float(dt))
        for n in (UMX, UMY, UMZ, UEDEN):
            s[n] += add[n]

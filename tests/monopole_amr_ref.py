"""numpy restatement of monopole gravity on AMR levels (tests only), written from the definitions in include/castro_hydro_amd.h:
the binning of a time-interpolated state, the level combination, the Gravity_Type boundary fill -- operation by operation, so
that they can be compared with the kernels exactly -- and a CPU backend that adds those methods of castro_amd.hydro.HipHydro to
tests/monopole_ref.MonopoleOracleBackend.  The coarse-fine interpolation of the gravity ghost zones is the backend's cc_interp
with 3 components.  The product never imports this file."""
import numpy as np

from tests import monopole_ref as R
from tests.monopole_ref import URHO, _sl


def interp_rho(rho_old, rho_new, omalpha, alpha):
    """S = S_old * omalpha; S_new * alpha; S = S + S_new: two rounded products, then the rounded sum"""
    a = np.asarray(rho_old, dtype=np.float64) * float(omalpha)
    b = np.asarray(rho_new, dtype=np.float64) * float(alpha)
    return a + b


def radial_mass_ex(boxes, geom, mono):
    """castro_amd_radial_mass_mf_ex.  boxes: [(rho_old, rho_new, lo, mask, omalpha, alpha)] of the valid zones; returns the dict of
    monopole_ref.radial_mass for the interpolated density (the rho == 0 test is made on it)"""
    return R.radial_mass([(interp_rho(ro, rn, oa, al), lo, mask) for ro, rn, lo, mask, oa, al in boxes], geom, mono)


def combine(arrays, n1ds, level):
    """castro_amd_radial_combine: arrays[lev] = (mass, vol) of level lev; returns (radial_mass_summed, radial_vol_summed) of `level`.
    Per fine bin: the level's own entry, then the coarser levels from level - 1 down to 0, each bin i < n1d / ratio of a coarser
    level spread over ratio fine bins as (1. / double(ratio)) * value."""
    n1d = int(n1ds[level])
    out = []
    for which in (0, 1):
        s = np.array(arrays[level][which][:n1d], dtype=np.float64)
        ratio = 1
        for lev in range(level - 1, -1, -1):
            ratio *= 2
            nc = n1d // ratio
            assert nc <= int(n1ds[lev]), "n1d / ratio exceeds the coarser array: CASTRO_AMD_ERR_UNSUPPORTED"
            w = 1. / float(ratio)
            s[:ratio * nc] += np.repeat(w * np.asarray(arrays[lev][which][:nc], dtype=np.float64), ratio)
        out.append(s)
    return out[0], out[1]


def grav_bc_fill(grav, box, geom):
    """castro_amd_grav_bc_fill_fab on grav (3, nz, ny, nx) over `box`, in place: a zone outside the domain in a non-periodic
    direction takes the zone its index maps to -- the nearest zone inside at inflow / outflow faces (bc 1, 2), the mirror image at
    symmetry faces and walls (bc >= 3) with the component normal to every mirrored face negated"""
    lo, hi = box
    src, flip, outside = [], [], []
    for d in range(3):
        idx = np.arange(lo[d], hi[d] + 1)
        s, f, o = idx.copy(), np.zeros(idx.shape, dtype=bool), np.zeros(idx.shape, dtype=bool)
        dl, dh = geom.domlo[d], geom.domhi[d]
        if geom.lo_bc[d] != 0:
            m = idx < dl
            o |= m
            if geom.lo_bc[d] >= 3:
                s[m], f[m] = 2 * dl - idx[m] - 1, True
            else:
                s[m] = dl
        if geom.hi_bc[d] != 0:
            m = idx > dh
            o |= m
            if geom.hi_bc[d] >= 3:
                s[m], f[m] = 2 * dh - idx[m] + 1, True
            else:
                s[m] = dh
        src.append(s - lo[d]); flip.append(f); outside.append(o)
    g = np.array(grav, copy=True)
    picked = g[:, src[2][:, None, None], src[1][None, :, None], src[0][None, None, :]]
    out_any = outside[2][:, None, None] | outside[1][None, :, None] | outside[0][None, None, :]
    for n in range(3):
        sh = [1, 1, 1]
        sh[2 - n] = -1
        v = np.where(flip[n].reshape(sh), -picked[n], picked[n])
        grav[n][out_any] = v[out_any]
    return out_any


class MonopoleAmrOracleBackend(R.MonopoleOracleBackend):
    """MonopoleOracleBackend + the methods of monopole gravity on AMR levels, in numpy (`ulps` moves the interpolated masses too)"""

    @staticmethod
    def make_radial_boxes(specs):
        return list(specs), len(specs)

    def radial_mass_mf_ex(self, boxes, omalpha, alpha, geom, mono, out, stream=None):
        specs, _ = boxes
        rb = []
        for lo, hi, (So, obox), (Sn, nbox), mask in specs:
            rb.append((So.numpy()[(URHO,) + _sl(obox, lo, hi)], Sn.numpy()[(URHO,) + _sl(nbox, lo, hi)], lo,
                       None if mask is None else mask.numpy(), omalpha, alpha))
        ref = radial_mass_ex(rb, geom, mono)
        mass = ref["mass"]
        for _ in range(abs(self.ulps)):
            mass = np.nextafter(mass, np.inf if self.ulps > 0 else -np.inf)
        o = out.numpy()
        o[:mono.n1d] = mass
        o[mono.n1d:] = ref["vol"]

    def radial_combine(self, level, mass_vols, n1ds, out, stream=None):
        arrs = [(mv.numpy()[:n], mv.numpy()[n:2 * n]) for mv, n in zip(mass_vols[:level + 1], n1ds[:level + 1])]
        m, v = combine(arrs, n1ds, level)
        n = int(n1ds[level])
        out.numpy()[:n] = m
        out.numpy()[n:2 * n] = v

    def grav_bc_fill(self, grav, grav_box, geom, stream=None):
        grav_bc_fill(grav.numpy(), grav_box, geom)


# ---- the dust-collapse hierarchy shared by the CPU and the GPU tests -------------------------------------------------------------
# the DUST_* case of monopole_ref.py on a 16^3 octant with a fixed 16^3 fine patch over the coarse zones (0,0,0)..(7,7,7), drdxfac 2
AMR_N, AMR_PATCH, AMR_DRDXFAC, AMR_STEPS = (16, 16, 16), ((0, 0, 0), (7, 7, 7)), 2, 2


def dust_amr_run(make_hydro, params, comm=None, do_grav=True, steps=AMR_STEPS, patches=None, **kw):
    """(hierarchy, [dt of every coarse step]) of the dust collapse on a refined hierarchy"""
    import castro_amd
    if patches is None:
        kw.setdefault("patch_crse", AMR_PATCH)
    else:
        kw["patches"] = patches
    g = castro_amd.MonopoleGravity(drdxfac=AMR_DRDXFAC, center=(0.0, 0.0, 0.0)) if do_grav else None
    a = castro_amd.CastroAmr(AMR_N, params=params, make_hydro=make_hydro, comm=comm, do_grav=do_grav, gravity=g, **R.DUST_GEOM, **kw)
    if not do_grav:
        for lev in a.lev:
            for b in lev.boxes:
                b.center = (0.0, 0.0, 0.0)
    a.initData("dust_collapse", **R.DUST_PROB)
    return a, [a.step() for _ in range(steps)]


def level_states(a):
    """[new-time state of the (single) box of every level] as numpy arrays"""
    return [lev.boxes[0].S_new().cpu().numpy() for lev in a.lev]


def dust_amr_sensitivity(oracle, **kw):
    """(reference hierarchy, its dts, s per level): the run on MonopoleAmrOracleBackend and the deviation per field that a second
    run shows whose radial masses differ by one ulp per bin (the rule of monopole_ref.dust_sensitivity)"""
    P = lambda: oracle.default_params(**R.DUST_PARAMS)
    ref, dts = dust_amr_run(lambda: MonopoleAmrOracleBackend(), P(), **kw)
    ulp, _ = dust_amr_run(lambda: MonopoleAmrOracleBackend(ulps=1), P(), **kw)
    s = [R.field_deviation(u, r) for u, r in zip(level_states(ulp), level_states(ref))]
    return ref, dts, s


# ---- the single-level driver against a hierarchy with no refined level: one route to the field ------------------------------------
def single_and_hierarchy(make_hydro, params, steps=2, **kw):
    """(Castro(gravity_type="monopole"), CastroAmr(gravity=MonopoleGravity(...)) with no refined level) after `steps` steps of the
    dust collapse"""
    import castro_amd
    c = castro_amd.Castro(AMR_N, params=params, hydro=make_hydro(), do_grav=True, gravity_type="monopole", drdxfac=AMR_DRDXFAC,
                          **R.DUST_GEOM, **kw)
    c.center = (0.0, 0.0, 0.0)
    c.initData("dust_collapse", **R.DUST_PROB)
    for _ in range(steps):
        c.step()
    a, _ = dust_amr_run(make_hydro, params, steps=steps, patches=[], **kw)
    return c, a


def assert_routes_agree_inside(c, a):
    """the same bits in S_new, in the radial arrays and in grav_old / grav_new on every zone inside the domain"""
    bits = lambda x: np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).view(np.int64)
    b = a.lev[0].boxes[0]
    assert len(a.lev) == 1 and c.nstep == a.nstep and c.time == a.time
    assert np.array_equal(bits(c.S_new()), bits(b.S_new()))
    for name in ("grav_old", "grav_new"):
        g = getattr(c, name)
        assert float(g.abs().max()) > 0.0
        assert np.array_equal(bits(g[:, 1:-1, 1:-1, 1:-1]), bits(getattr(b, name)[:, 1:-1, 1:-1, 1:-1])), name
    (m, v, g), (am, av, _, agn) = c.radial_gravity(), a.gravity.radial_gravity(0)
    assert m.shape == (c.n1d,) and m.sum() > 0.0
    for x, y in ((m, am), (v, av), (g, agn)):
        assert np.array_equal(bits(x), bits(y))


def assert_ghost_zone_is_the_interpolation(c, exact):
    """grav_new of a single-level Castro with monopole gravity: the ghost zone outside the domain holds the monopole
    interpolation at that zone's own radius, not the Gravity_Type fill of the interior (the f-row of monopole
    gravity).  exact: bit for bit; else within 1e-10 of the largest radial gravity (the bound of the interpolation kernel's test)"""
    from castro_amd import _lib
    rg = c.radial_gravity()[2]
    mono = _lib.make_monopole(c.n_cell, c.geom, getattr(c, "center", None) or [0.5 * (c.geom.problo[d] + c.geom.probhi[d]) for d in range(3)],
                              c.drdxfac, c.Gconst)
    got = c.grav_new.cpu().numpy()
    want = np.full(got.shape, np.nan)
    index = R.interpolate(rg, c.geom, mono, want, c.gravbox)
    ghost = np.ones(got.shape[1:], dtype=bool)
    ghost[1:-1, 1:-1, 1:-1] = False
    ghost &= index <= mono.n1d - 1
    assert ghost.sum() > 0.9 * (18 ** 3 - 16 ** 3)
    if exact:
        assert np.array_equal(got[:, ghost], want[:, ghost])
    else:
        assert np.abs(got - want)[:, ghost].max() <= 1e-10 * np.abs(rg).max()
    filled = got.copy()
    grav_bc_fill(filled, c.gravbox, c.geom)
    assert np.abs(got - filled)[:, ghost].max() > 1e-6 * np.abs(rg).max(), "not the extrapolated / reflected interior value"

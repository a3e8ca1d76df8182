"""gravity.gravity_type = "MonopoleGrav" on the levels of CastroAmr: the part of the reference's Gravity object that spans the levels
(Source/gravity/Gravity.cpp).  castro_amd.CastroAmr(do_grav=True, gravity=MonopoleGravity(drdxfac=..., Gconst=...)).

  make_radial_gravity(level, time)   Gravity::make_radial_gravity (:2962-3274): every level lev <= level binned at `time` -- old,
                                     new or time-interpolated data (the eps tests of :2966-3001), the zones under level lev + 1
                                     masked for lev < level --, one sum over the ranks per level array, the level combination
                                     of :3103-3168 and the outward integration, all on the device
  get_old_grav_vector(level) /       Gravity::get_old_grav_vector / get_new_grav_vector (:832-973): make_radial_gravity at the
  get_new_grav_vector(level)         level's old / new time, interpolate_monopole_grav onto grav_old / grav_new of every box of
                                     the level, then the FillPatch of Gravity_Type (_Level.fill_grav: coarse data interpolated in
                                     time and space, siblings, physical boundaries)

  PointMass                          castro.use_point_mass / castro.point_mass / castro.point_mass_fix_solution: a mass M at
                                     problem::center, ONE device double per run (per CastroAmr hierarchy: castro::point_mass is
                                     one global shared by the levels).  add(): Gravity::add_pointmass_to_gravity (:2903-2948) over
                                     the grown gravity FABs, called at the END of get_old / get_new_grav_vector (:902-907,
                                     :975-980) -- after the interpolation and after the Gravity_Type FillPatch, so a coarse-fine
                                     ghost zone of a refined level holds the coarse level's data, which already carry the coarse
                                     level's point-mass term, PLUS the level's own term: the reference's result, reproduced.
                                     update(): Castro::pointmass_update (Source/gravity/Castro_pointmass.cpp), two launches with
                                     the sum over the ranks between them and no host round trip.

  PoissonGravity                     gravity.gravity_type = "PoissonGrav" on a single level (castro_amd.Castro(poisson=...)): the
                                     multipole boundary values, the multigrid solve and g = -grad(phi) of one time level, and the
                                     old / new potentials of the run (the class at the end of this file); and on the levels of
                                     CastroAmr (gravity=PoissonGravity(...)) in the reference's level-solve configuration
                                     (gravity.no_sync = 1, gravity.no_composite = 1, gravity.max_solve_level): every level solves on
                                     its own box, a refined one with Dirichlet data from the level below at its own time.

Levels finer than `level` do not enter.  Not provided with monopole gravity: GR_GRAV, gravity.max_solve_level, a potential (phiGrav), domains with a periodic direction (the Gravity_Type FillPatch across a periodic boundary is not built), thermal
diffusion on AMR levels, constant gravity plus a point mass on AMR levels.
"""
from . import _lib as L


def time_branch(time, t_old, t_new):
    """Which data of a level make_radial_gravity bins at `time` (Gravity.cpp:2966-3004): ("new", 1.0) | ("old", 0.0) |
    ("interp", alpha) with alpha = (time - t_old) / (t_new - t_old); outside [t_old, t_new] the reference aborts."""
    eps = (t_new - t_old) * 1.e-6
    if eps == 0.0:
        return "new", 1.0
    if abs(time - t_old) < eps:
        return "old", 0.0
    if abs(time - t_new) < eps:
        return "new", 1.0
    if time > t_old and time < t_new:
        return "interp", (time - t_old) / (t_new - t_old)
    raise RuntimeError("Problem in Gravity::make_radial_gravity: time %r is outside the level's old / new times %r / %r"
                       % (time, t_old, t_new))


class PointMass:
    """The central point mass of a run.  buf: two device doubles, [point_mass, mass_change_at_center]."""

    def __init__(self, hydro, mass, fix_solution=False, Gconst=L.GCONST):
        for name in ("add_pointmass_mf", "pointmass_delta_mf", "pointmass_apply_mf"):
            if not hasattr(hydro, name):
                raise RuntimeError("castro_amd: this backend has no %s; there is no host fallback" % name)
        self.fix_solution, self.Gconst = bool(fix_solution), float(Gconst)
        self.buf = hydro.alloc(1, (0, 0, 0), (1, 0, 0)).reshape(2)
        self.buf[0] = float(mass)
        self.mass, self.delta = self.buf[:1], self.buf[1:]
        self.nupdates = 0                       # pointmass_update calls that ran (whatever the sign of the change)

    def value(self):
        """the point mass as the device holds it (one copy to the host)"""
        return float(self.buf[0])

    def params(self, center):
        return L.make_pointmass(center, self.Gconst)

    def add(self, hydro, fabs, center, geom):
        """Gravity::add_pointmass_to_gravity over every FAB of `fabs` (HipHydro.make_grav_fabs): their whole boxes"""
        hydro.add_pointmass_mf(fabs, self.params(center), geom, self.mass)

    def update(self, hydro, comm, boxes, center, geom):
        """Castro::pointmass_update over `boxes` (HipHydro.make_pointmass_boxes): the caller has checked level == finest_level
        and point_mass_fix_solution"""
        pm = self.params(center)
        hydro.pointmass_delta_mf(boxes, pm, geom, self.delta)
        comm.allreduce_sum(self.delta)          # ParallelDescriptor::ReduceRealSum(mass_change_at_center)
        hydro.pointmass_apply_mf(boxes, pm, geom, self.delta, self.mass)
        self.nupdates += 1


class MonopoleGravity:
    def __init__(self, drdxfac=1, Gconst=L.GCONST, center=None):
        """drdxfac: gravity.drdxfac; Gconst: the reference takes C::Gconst from its Microphysics constants (the default is the cgs
        value of that release); center: problem::center, default the middle of the domain."""
        self.drdxfac, self.Gconst = int(drdxfac), float(Gconst)
        self.center = None if center is None else tuple(float(x) for x in center)
        if self.drdxfac < 1:
            raise ValueError("gravity.drdxfac must be at least 1, not %d" % self.drdxfac)
        self.amr = None
        self.point_mass = None                  # the PointMass of the hierarchy (CastroAmr(use_point_mass=True))
        self._lev = {}

    # ---- the hierarchy this object belongs to ---------------------------------------------------------------
    def bind(self, amr, lo_bc, hi_bc):
        if any(lo_bc[d] == 0 or hi_bc[d] == 0 for d in range(3)):
            raise (ValueError if all(lo_bc[d] == 0 and hi_bc[d] == 0 for d in range(3)) else NotImplementedError)(
                "monopole gravity needs a non-periodic domain: a fully periodic one has no isolated mass to take the radial "
                "profile of, and the Gravity_Type FillPatch across a periodic boundary of a partly periodic one is not built")
        if self.amr is not None and self.amr is not amr:
            raise ValueError("a MonopoleGravity object belongs to one CastroAmr")
        self.amr = amr

    def check_level(self, l, geom):
        """the checks of the single-level driver with this level's dx"""
        dmax = L.monopole_max_drdxfac([geom.dx[d] for d in range(3)])
        if self.drdxfac > dmax:
            raise ValueError("gravity.drdxfac = %d is above the %d the geometry of level %d allows: the binning kernel holds the "
                             "sub-zones of a brick of 8 x 8 x 4 zones in a window of 64 bins (drdxfac <= 5 for cubic zones)"
                             % (self.drdxfac, dmax, l))
        if l >= L.MONOPOLE_MAX_LEVELS:
            raise ValueError("monopole gravity: at most %d levels" % L.MONOPOLE_MAX_LEVELS)

    def reset(self, from_level=0):
        """regrid / _push_level / _drop_fine: the box tables and masks of levels >= from_level - 1 hold pointers into boxes that
        are gone, or describe a coverage that has changed"""
        for l in list(self._lev):
            if l >= from_level:
                del self._lev[l]
            else:
                self._lev[l]["tables"] = {}

    def n1d(self, l):
        """bins of level l: monopole_n1d of the level's domain (Gravity.cpp:315, Castro.cpp:3887-3913)"""
        return L.monopole_n1d(tuple((2 ** l) * x for x in self.amr.n_cell), self.drdxfac)

    def problem_center(self):
        if self.center is not None:
            return list(self.center)
        g = self.amr.lev[0].geom
        return [0.5 * (g.problo[d] + g.probhi[d]) for d in range(3)]

    def params(self, l):
        """castro_amd_monopole_params of level l"""
        lev = self.amr.lev[l]
        return L.make_monopole(tuple((2 ** l) * x for x in self.amr.n_cell), lev.geom, self.problem_center(), self.drdxfac,
                               self.Gconst, n1d=self.n1d(l))

    def _arrays(self, l):
        """radial_mass / radial_vol of level l (one array of 2 n1d), the combined arrays, radial_grav_old / radial_grav_new"""
        ent = self._lev.get(l)
        if ent is None:
            h, n = self.amr.lev[l].hydro, self.n1d(l)
            vec = lambda m: h.alloc(1, (0, 0, 0), (m - 1, 0, 0)).reshape(-1)
            ent = self._lev[l] = dict(mv=vec(2 * n), summed=vec(2 * n), old=vec(n), new=vec(n), tables={})
        return ent

    # ---- Gravity::make_radial_gravity ---------------------------------------------------------------------------
    def _bin_level(self, lev_i, level, time, which):
        """radial_mass[lev_i], radial_vol[lev_i] at `time`, summed over the ranks"""
        amr = self.amr
        lev = amr.lev[lev_i]
        h = lev.hydro
        ent = self._arrays(lev_i)
        if lev_i == level:
            branch, alpha = ("old", 0.0) if which == "old" else ("new", 1.0)       # the level's own advance: its own old / new data
        else:
            branch, alpha = time_branch(time, lev.t_old, lev.t_new)
        masks = amr._diag_level_masks(lev_i) if lev_i < level else None
        mkey = tuple(m.data_ptr() for m in (masks or {}).values())
        mask_of = lambda b: masks[b.bx] if masks is not None else None
        tables = ent["tables"]
        if len(tables) > 32:
            tables.clear()
        geom, mono = lev.geom, self.params(lev_i)
        if branch == "interp":
            if not hasattr(h, "radial_mass_mf_ex"):
                raise RuntimeError("castro_amd: this backend has no radial_mass_mf_ex; there is no host fallback")
            key = ("ex", mkey) + tuple(t.data_ptr() for b in lev.mine for t in (b.S_old_b, b.S_new_b))
            if key not in tables:
                tables[key] = h.make_radial_boxes([(b.lo, b.hi, (b.S_old_b, b.gbox), (b.S_new_b, b.gbox), mask_of(b)) for b in lev.mine])
            h.radial_mass_mf_ex(tables[key], 1.0 - alpha, alpha, geom, mono, ent["mv"])
        else:
            name = "S_old_b" if branch == "old" else "S_new_b"
            key = (name, mkey) + tuple(getattr(b, name).data_ptr() for b in lev.mine)
            if key not in tables:
                tables[key] = h.make_diag_boxes([(b.lo, b.hi, (getattr(b, name), b.gbox), mask_of(b)) for b in lev.mine])
            h.radial_mass_mf(tables[key], geom, mono, ent["mv"])
        amr.comm.allreduce_sum(ent["mv"])               # ParallelDescriptor::ReduceRealSum of the level's arrays
        return branch

    def make_radial_gravity(self, level, time, which="new"):
        """radial_grav_old[level] (which = "old") or radial_grav_new[level] at `time`; returns the data each level was binned
        from ("old" | "new" | "interp"), coarsest first"""
        branches = [self._bin_level(l, level, time, which) for l in range(level + 1)]
        h = self.amr.lev[level].hydro
        ent = self._arrays(level)
        if level == 0:
            summed = ent["mv"]
        else:
            if not hasattr(h, "radial_combine"):
                raise RuntimeError("castro_amd: this backend has no radial_combine; there is no host fallback")
            summed = ent["summed"]
            h.radial_combine(level, [self._arrays(l)["mv"] for l in range(level + 1)], [self.n1d(l) for l in range(level + 1)], summed)
        ent["last_summed"] = summed
        h.radial_gravity(self.params(level), self.amr.lev[level].geom, summed, ent[which])
        return branches

    # ---- Gravity::get_old_grav_vector / get_new_grav_vector -----------------------------------------------------
    def _grav_vector(self, level, which, time, a):
        lev = self.amr.lev[level]
        self.make_radial_gravity(level, time, which)
        rg, mono = self._arrays(level)[which], self.params(level)
        name = "grav_" + which
        for b in lev.mine:
            lev.hydro.monopole_grav(rg, mono, lev.geom, getattr(b, name), b.gravbox)
        lev.fill_grav(name, a)
        if self.point_mass is not None and lev.mine:
            # add_pointmass_to_gravity comes last (Gravity.cpp:902-907, 975-980): on top of whatever the FillPatch has put into
            # the ghost zones -- on a refined level the coarse data with the coarse level's point-mass term
            h = lev.hydro
            fabs = h.make_grav_fabs([(getattr(b, name), b.gravbox) for b in lev.mine])       # descriptors are memoised
            self.point_mass.add(h, fabs, self.problem_center(), lev.geom)

    def get_old_grav_vector(self, level, time=None, a=0.0):
        """grav_old of every box of `level` at the level's old time; a: where that time lies in the parent's [old, new]"""
        self._grav_vector(level, "old", self.amr.lev[level].t_old if time is None else time, a)

    def get_new_grav_vector(self, level, time=None, a=1.0):
        self._grav_vector(level, "new", self.amr.lev[level].t_new if time is None else time, a)

    def radial_gravity(self, level):
        """(radial_mass_summed, radial_vol_summed, radial_grav_old, radial_grav_new) of `level` after its last construction, numpy"""
        ent, n = self._arrays(level), self.n1d(level)
        mv = ent.get("last_summed", ent["mv"]).cpu().numpy()
        return mv[:n].copy(), mv[n:].copy(), ent["old"].cpu().numpy().copy(), ent["new"].cpu().numpy().copy()


class PoissonGravity:
    """gravity.gravity_type = "PoissonGrav" on a single level: castro_amd.Castro(do_grav=True, poisson=PoissonGravity(...)).

    Every construction of the gravity of a time level (Castro::construct_old_gravity / construct_new_gravity,
    Source/gravity/Castro_gravity.cpp) is: the multipole moments of the valid zones of the state (Gravity::fill_multipole_BCs),
    the boundary potential on the ghost shell of phi, the multigrid solve of lap(phi) = 4 pi G rho from the level's starting
    guess, g = -grad(phi) on the valid zones, and the Gravity_Type boundary fill of the ghost zone of g.  Time levels: at the
    start of a step phi_old <- phi_new; the old-time solve starts from phi_old, the new-time solve from a copy of phi_old
    (Castro_gravity.cpp:146); the first solve of a run starts from zero.  The reference's extra solve in post_init is not made.

    max_multipole_order: gravity.max_multipole_order (lnum); reltol / abstol: gravity.rel_tol / abs_tol of the stopping rule
    ||r|| <= max(reltol ||b||, abstol max(b)); maxiter: V-cycles before RuntimeError (the reference aborts there); Gconst:
    C::Gconst; center: problem::center, default the driver's `center`, else the middle of the domain.
    Not built (each refused by the driver): more than one rank, periodic or Symmetry faces, the point mass,
    checkpoints, gravity.mlmg_maxorder > 2, direct_sum_bcs.

    On a hierarchy: castro_amd.CastroAmr(do_grav=True, gravity=PoissonGravity(..., max_solve_level=None)) -- the level solves of
    the second half of this class.  max_solve_level: gravity.max_solve_level, the finest level that solves (None: every level, the
    reference's default); a finer level takes phi and g from the level below by interpolation.  no_sync / no_composite:
    gravity.no_sync / gravity.no_composite; only True is built (no composite solve, no gravity_sync, no composite correction).
    One rank, refinement ratio 2, level 0 and every refined level ONE box, the refined ones inside the domain."""

    OPERATIONS = ("multipole_moments_mf", "multipole_phi_bc", "poisson_solve", "grad_phi_to_grav")
    AMR_OPERATIONS = ("poisson_cf_bc", "lincomb", "cc_interp")
    drdxfac = 1                                 # a box of a CastroAmr level copies it from its gravity object; not used here

    def __init__(self, max_multipole_order=0, reltol=1.e-10, abstol=1.e-10, maxiter=40, Gconst=L.GCONST, center=None,
                 max_solve_level=None, no_sync=True, no_composite=True):
        if not no_sync or not no_composite:
            raise NotImplementedError("Poisson gravity: gravity.no_sync = 0 / gravity.no_composite = 0 -- the composite solve, "
                                      "gravity_sync and the composite correction of the hierarchy -- are not built; the levels "
                                      "solve for themselves (no_sync=True, no_composite=True)")
        self.max_solve_level = None if max_solve_level is None else int(max_solve_level)
        if self.max_solve_level is not None and self.max_solve_level < 0:
            raise ValueError("gravity.max_solve_level must not be negative, not %d" % self.max_solve_level)
        self.amr = None
        self.point_mass = None
        self._lev = {}
        self.solve_log = []                     # (level, "old" | "new", a) of the last solves of a hierarchy, oldest first
        self.lnum = int(max_multipole_order)
        if self.lnum < 0:
            raise ValueError("gravity.max_multipole_order must not be negative, not %d" % self.lnum)
        if self.lnum > L.MAX_MULTIPOLE:
            raise ValueError("gravity.max_multipole_order = %d is above the %d the kernels are built for (the reference's "
                             "lnum_max is 30): a follow-up raises CASTRO_AMD_MAX_MULTIPOLE" % (self.lnum, L.MAX_MULTIPOLE))
        self.reltol, self.abstol, self.maxiter = float(reltol), float(abstol), int(maxiter)
        self.Gconst = float(Gconst)
        self.center = None if center is None else tuple(float(x) for x in center)
        self.driver = None
        self.plan = None
        self.stats = {"first": None, "old": None, "new": None}

    def bind(self, owner, *args):
        """bind(castro, hydro_alloc): the single-level driver (Castro(poisson=...)); bind(amr, lo_bc, hi_bc): the hierarchy
        (CastroAmr(gravity=...), the call MonopoleGravity answers too)"""
        if len(args) == 1:
            return self._bind_single(owner, args[0])
        lo_bc, hi_bc = args
        if self.driver is not None or (self.amr is not None and self.amr is not owner):
            raise ValueError("a PoissonGravity object belongs to one Castro or one CastroAmr")
        self._refuse_faces(lo_bc, hi_bc)
        self.amr = owner

    @staticmethod
    def _refuse_faces(lo_bc, hi_bc):
        for d in range(3):
            for bc in (lo_bc[d], hi_bc[d]):
                if bc == 0 or bc == 3:
                    raise NotImplementedError("Poisson gravity with a %s face: the mass offset of a periodic domain and the "
                                              "reflected moments / Neumann faces of a Symmetry one are a follow-up; all six faces "
                                              "must be Dirichlet faces of the potential" % ("periodic" if bc == 0 else "Symmetry"))

    def _bind_single(self, c, hydro_alloc):
        """the checks of the driver `c` this object belongs to, and its arrays: phi_old / phi_new with one ghost zone, the moments"""
        if self.amr is not None or (self.driver is not None and self.driver is not c):
            raise ValueError("a PoissonGravity object belongs to one Castro")
        h = c.hydro
        missing = [name for name in self.OPERATIONS + ("poisson_plan_create", "grav_bc_fill") if not hasattr(h, name)]
        if missing:
            raise NotImplementedError("Poisson gravity: this backend has no %s; there is no host fallback" % ", ".join(missing))
        for d in range(3):
            for bc in (c.lo_bc[d], c.hi_bc[d]):
                if bc == 0 or bc == 3:
                    raise NotImplementedError("Poisson gravity with a %s face: the mass offset of a periodic domain and the "
                                              "reflected moments / Neumann faces of a Symmetry one are a follow-up; all six faces "
                                              "must be Dirichlet faces of the potential" % ("periodic" if bc == 0 else "Symmetry"))
        coarsest = L.poisson_level_extents(c.n_cell)[-1]
        if coarsest[0] * coarsest[1] * coarsest[2] > L.POISSON_MAX_BOTTOM:
            raise ValueError("Poisson gravity: n_cell = %s coarsens to %s, more than the %d zones the bottom solver of the multigrid "
                             "takes: n_cell needs more factors of 2" % (c.n_cell, coarsest, L.POISSON_MAX_BOTTOM))
        self.driver = c
        self.phibox = (tuple(x - 1 for x in c.lo), tuple(x + 1 for x in c.hi))
        self.phi_old = hydro_alloc(1, *self.phibox)
        self.phi_new = hydro_alloc(1, *self.phibox)
        n1 = self.lnum + 1
        self.moments = hydro_alloc(1, (0, 0, 0), (3 * n1 * n1 - 1, 0, 0))
        self._tables = {}
        if self.phi_old is not None:
            self.plan = h.poisson_plan_create(c.geom)

    def close(self):
        if self.plan is not None and self.driver is not None:
            self.driver.hydro.poisson_plan_destroy(self.plan)
        self.plan = None
        for ent in self._lev.values():          # the plans of a hierarchy; phi stays, a later solve makes the plan again
            self._free_plan(ent)

    @staticmethod
    def _free_plan(ent):
        if ent.get("plan") is not None:
            ent["hydro"].poisson_plan_destroy(ent["plan"])
        ent["plan"] = None

    def __del__(self):
        try:
            # a finaliser that runs in the middle of a stream capture must not free device memory (HipHydro.__del__)
            import torch
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                return
            self.close()
        except Exception:
            pass

    def swap_time_levels(self):
        """swap_state_time_levels of PhiGrav_Type: the new data of the last step are the old data of this one"""
        self.phi_old, self.phi_new = self.phi_new, self.phi_old

    def multipole(self):
        """castro_amd_multipole of the run"""
        from . import diag
        c = self.driver
        return L.make_multipole(c.geom, self.center if self.center is not None else diag.domain_center(c), self.lnum, self.Gconst)

    def construct(self, S, grav, new):
        """Gravity::solve_for_phi and get_old / get_new_grav_vector of the level at one time level: `grav` from the state S"""
        import math
        c = self.driver
        h = c.hydro
        if self.plan is None:                           # after Castro.close(): the plan is made again
            self.plan = h.poisson_plan_create(c.geom)
        if new:
            self.phi_new.copy_(self.phi_old)            # the "old" phi of the step is the guess (Castro_gravity.cpp:146)
        phi = self.phi_new if new else self.phi_old
        mp = self.multipole()
        key = S.data_ptr()                              # the two state buffers swap roles every step: one table each
        if key not in self._tables:
            self._tables[key] = h.make_diag_boxes([(c.lo, c.hi, (S, c.gbox), None)])
        mom = self.moments.reshape(-1)
        h.multipole_moments_mf(self._tables[key], c.geom, mp, mom)
        h.multipole_phi_bc(phi, self.phibox, c.geom, mp, mom)
        cycles, ok, norm, hist = h.poisson_solve(self.plan, phi, self.phibox, S, c.gbox, L.URHO, 4.0 * math.pi * self.Gconst,
                                                 self.reltol, self.abstol, self.maxiter)
        self.stats["new" if new else "old"] = {"cycles": cycles, "norm": norm, "history": hist}
        if self.stats["first"] is None:
            self.stats["first"] = self.stats["new" if new else "old"]
        if not ok:
            raise RuntimeError("Poisson gravity: the multigrid did not reach max(%g * %g, %g * %g) in %d V-cycles; the last two "
                               "residual norms are %r and %r" % (self.reltol, hist[0], self.abstol, hist[1], self.maxiter,
                                                                  hist[-2], hist[-1]))
        h.grad_phi_to_grav(phi, self.phibox, grav, c.gravbox, c.geom)
        h.grav_bc_fill(grav, c.gravbox, c.geom)

    # ---- the levels of a CastroAmr hierarchy: level solves (gravity.no_sync = 1, gravity.no_composite = 1) -----------------
    # Castro::construct_old_gravity / construct_new_gravity (Castro_gravity.cpp:14-232) and Gravity::solve_for_phi /
    # get_old_grav_vector / get_new_grav_vector / GetCrsePhi (Gravity.cpp:418-485, 664-690, 838-981) on a hierarchy whose refined
    # levels are one box each.  Level 0 is the single-level path above.  A level 0 < l <= max_solve_level solves on its own box
    # -- a geometry whose domain is the box goes to the same entry points -- with Dirichlet data from the potential of the level
    # below at its own time (castro_amd_poisson_cf_bc_fab).  A level above max_solve_level takes phi and g of its whole FABs from
    # the level below (FillCoarsePatch: lincomb in time, cc_interp in space).
    def solves(self, level):
        return self.max_solve_level is None or level <= self.max_solve_level

    def check_level(self, l, geom):
        h = self.amr._hydro_for(l)
        missing = [name for name in self.OPERATIONS + self.AMR_OPERATIONS + ("poisson_plan_create", "grav_bc_fill") if not hasattr(h, name)]
        if missing:
            raise NotImplementedError("Poisson gravity: this backend has no %s; there is no host fallback" % ", ".join(missing))
        if l == 0:
            n = tuple(geom.domhi[d] - geom.domlo[d] + 1 for d in range(3))
            self._check_bottom(0, (tuple(geom.domlo[d] for d in range(3)), tuple(geom.domhi[d] for d in range(3))), n)

    def _check_bottom(self, l, box, n):
        coarsest = L.poisson_level_extents(n)[-1]
        if coarsest[0] * coarsest[1] * coarsest[2] > L.POISSON_MAX_BOTTOM:
            raise ValueError("Poisson gravity: the box %s of level %d (%s zones) coarsens to %s, more than the %d zones the bottom "
                             "solver of the multigrid takes (CASTRO_AMD_POISSON_MAX_BOTTOM): its extents need more factors of 2 "
                             "-- a blocking_factor of 16 or 32" % (box, l, n, coarsest, L.POISSON_MAX_BOTTOM))

    def check_boxes(self, l, boxes, parents):
        """the boxes (lo, hi) of the refined level l about to be made, in its own zones; parents: those of level l - 1"""
        if len(boxes) != 1 or len(parents) != 1:
            raise NotImplementedError("Poisson gravity: level %d would have %d boxes (level %d has %d) -- the level solves are "
                                      "built for refined levels of ONE box; a level of several boxes needs the halo exchange of "
                                      "phi between them" % (l, len(boxes), l - 1, len(parents)))
        lo, hi = boxes[0]
        dom = tuple((2 ** l) * x for x in self.amr.n_cell)
        if any(lo[d] <= 0 or hi[d] >= dom[d] - 1 for d in range(3)):
            raise NotImplementedError("Poisson gravity: the box %s of level %d touches the domain boundary -- the multipole "
                                      "boundary values of a refined level are not built; the box must lie inside the domain"
                                      % ((lo, hi), l))
        if not self.solves(l):
            return
        plo, phi = parents[0]
        if any((lo[d] >> 1) - 1 < plo[d] or (hi[d] >> 1) + 1 > phi[d] for d in range(3)):
            raise ValueError("Poisson gravity: the box %s of level %d, coarsened and grown by one zone, does not lie inside the "
                             "valid box %s of level %d: its boundary values would read ghost zones of the coarse potential"
                             % ((lo, hi), l, (plo, phi), l - 1))
        self._check_bottom(l, (lo, hi), tuple(hi[d] - lo[d] + 1 for d in range(3)))

    def reset(self, from_level=0):
        """regrid / _push_level / _drop_fine: the levels >= from_level are gone or re-made -- their potentials and plans go"""
        for l in list(self._lev):
            if l >= from_level:
                self._free_plan(self._lev[l])
                del self._lev[l]

    def problem_center(self):
        if self.center is not None:
            return list(self.center)
        g = self.amr.lev[0].geom
        return [0.5 * (g.problo[d] + g.probhi[d]) for d in range(3)]

    def _entry(self, l):
        """phi_old / phi_new (one ghost zone), the plan and the scratch of level l, made for the box the level has now"""
        lev = self.amr.lev[l]
        b = lev.mine[0]
        ent = self._lev.get(l)
        if ent is not None and ent["key"] != b.bx:       # a plan is kept per level, keyed by the extents of its box
            self._free_plan(ent)
            ent = None
        if ent is None:
            h = lev.hydro
            phibox = (tuple(x - 1 for x in b.lo), tuple(x + 1 for x in b.hi))
            ent = self._lev[l] = dict(key=b.bx, hydro=h, phibox=phibox, phi_old=h.alloc(1, *phibox), phi_new=h.alloc(1, *phibox),
                                      plan=None, have=(l == 0), tables={}, stats={"first": None, "old": None, "new": None})
            if l == 0:
                n1 = self.lnum + 1
                ent["moments"] = h.alloc(1, (0, 0, 0), (3 * n1 * n1 - 1, 0, 0))
                ent["geom"] = lev.geom
            else:
                g = L.Geom.from_buffer_copy(lev.geom)    # the level's dx and problo; the "domain" is the box, Dirichlet all round
                for d in range(3):
                    g.domlo[d], g.domhi[d], g.lo_bc[d], g.hi_bc[d] = b.lo[d], b.hi[d], 2, 2
                ent["geom"] = g
                # coarse zones under the box grown by one, grown by one more for the slopes of cc_interp
                ent["cbox"] = (tuple((x >> 1) - 2 for x in b.lo), tuple((x >> 1) + 2 for x in b.hi))
                ent["ctmp"] = h.alloc(1, *ent["cbox"])
        return ent

    def swap_level(self, l):
        """swap_state_time_levels of PhiGrav_Type of level l, at the start of every advance of the level"""
        ent = self._lev.get(l)
        if ent is not None:
            ent["phi_old"], ent["phi_new"] = ent["phi_new"], ent["phi_old"]

    def _crse_at(self, l, ent, a):
        """GetCrsePhi: (1 - a) phi_old + a phi_new of level l - 1 into the scratch of level l, where level l - 1 has data"""
        P = self._entry(l - 1)
        cb, pb = ent["cbox"], P["phibox"]
        lo = tuple(max(cb[0][d], pb[0][d]) for d in range(3))
        hi = tuple(min(cb[1][d], pb[1][d]) for d in range(3))
        ent["hydro"].lincomb(ent["ctmp"], cb, 1.0 - a, P["phi_old"], pb, a, P["phi_new"], pb, 1, lo, hi)
        return P

    def _grav_vector(self, level, which, a):
        import math
        lev = self.amr.lev[level]
        b = lev.mine[0]
        h = lev.hydro
        ent = self._entry(level)
        name = "grav_" + which
        grav = getattr(b, name)
        phi, pbx = ent["phi_" + which], ent["phibox"]
        if level > 0 and not self.solves(level):
            # no solve above max_solve_level: phi and g of the whole FABs are the FillCoarsePatch of the level below
            # (Gravity.cpp:466, 846-852, 919-925)
            self._crse_at(level, ent, a)
            h.cc_interp(ent["ctmp"], ent["cbox"], phi, pbx, pbx[0], pbx[1], 1)
            ent["have"] = True
            for p, (lo, hi) in b.gsrc + b.gsrc_valid:
                h.lincomb(b.gctmp, b.gcbox, 1.0 - a, p.grav_old, p.gravbox, a, p.grav_new, p.gravbox, 3, lo, hi)
            h.cc_interp(b.gctmp, b.gcbox, grav, b.gravbox, b.gravbox[0], b.gravbox[1], 3)
            return
        if not ent["have"]:
            # the first solve of the level, or of a level a regrid has re-made: the level below, interpolated, is the guess
            self._crse_at(level, ent, a)
            h.cc_interp(ent["ctmp"], ent["cbox"], phi, pbx, b.lo, b.hi, 1)
            ent["have"] = True
        elif which == "new":
            phi.copy_(ent["phi_old"])                    # the "old" phi of the step is the guess (Castro_gravity.cpp:146)
        if ent["plan"] is None:                          # the first solve, or after close()
            ent["plan"] = h.poisson_plan_create(ent["geom"])
        S = b.S_old_b if which == "old" else b.S_new_b
        if level == 0:
            geom = ent["geom"]
            mp = L.make_multipole(geom, self.problem_center(), self.lnum, self.Gconst)
            key = S.data_ptr()
            if key not in ent["tables"]:
                ent["tables"][key] = h.make_diag_boxes([(b.lo, b.hi, (S, b.gbox), None)])
            mom = ent["moments"].reshape(-1)
            h.multipole_moments_mf(ent["tables"][key], geom, mp, mom)      # fill_multipole_BCs(level, level): this level alone
            h.multipole_phi_bc(phi, pbx, geom, mp, mom)
        else:
            P = self._lev[level - 1]
            h.poisson_cf_bc(phi, pbx, b.lo, b.hi, P["phi_old"], P["phibox"], P["phi_new"], P["phibox"], a)
        cycles, ok, norm, hist = h.poisson_solve(ent["plan"], phi, pbx, S, b.gbox, L.URHO, 4.0 * math.pi * self.Gconst,
                                                 self.reltol, self.abstol, self.maxiter)
        st = ent["stats"]
        st[which] = {"cycles": cycles, "norm": norm, "history": hist}
        if st["first"] is None:
            st["first"] = st[which]
        self.solve_log.append((level, which, a))
        del self.solve_log[:-256]
        if not ok:
            raise RuntimeError("Poisson gravity, level %d: the multigrid did not reach max(%g * %g, %g * %g) in %d V-cycles; the "
                               "last two residual norms are %r and %r" % (level, self.reltol, hist[0], self.abstol, hist[1],
                                                                          self.maxiter, hist[-2], hist[-1]))
        h.grad_phi_to_grav(phi, pbx, grav, b.gravbox, ent["geom"])
        lev.fill_grav(name, a)                           # the Gravity_Type FillPatch of the ghost zones of g

    def get_old_grav_vector(self, level, time=None, a=0.0):
        """phi_old and grav_old of `level` at the level's old time; a: where that time lies in the parent's [old, new]"""
        self._grav_vector(level, "old", a)

    def get_new_grav_vector(self, level, time=None, a=1.0):
        self._grav_vector(level, "new", a)

    def phi_level(self, level, new=True):
        return self._entry(level)["phi_new" if new else "phi_old"]

    def stats_level(self, level):
        return dict(self._entry(level)["stats"])

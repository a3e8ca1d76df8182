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

  PoissonGravity                     gravity.gravity_type = "PoissonGrav" in the reference's level-solve configuration
                                     (gravity.no_sync = 1, gravity.no_composite = 1, gravity.max_solve_level): every level solves on
                                     its own box or boxes -- level 0 with multipole boundary values, a refined one with Dirichlet
                                     data from the level below at its own time; a level of several boxes as one array over their
                                     bounding box --, then g = -grad(phi); the old / new potentials per level.

  ConstantGravity                    ConstantGrav as Gravity_Type data, for the one case that needs them: a point mass on top.

  SingleLevel                        castro_amd.Castro as a hierarchy of one level: the single-level driver gets its gravity field
                                     from the same objects, through the same calls, as the levels of CastroAmr.

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


class SingleLevel:
    """A single-level castro_amd.Castro as the gravity objects see a CastroAmr: the hierarchy and its level 0 in one object
    (amr.lev[0] is amr), with the driver as the level's one box."""

    def __init__(self, castro):
        self.mine = [castro]
        self.lev = [self]

    n_cell = property(lambda self: self.mine[0].n_cell)
    comm = property(lambda self: self.mine[0].comm)
    hydro = property(lambda self: self.mine[0].hydro)
    geom = property(lambda self: self.mine[0].geom)
    center = property(lambda self: getattr(self.mine[0], "center", None))      # may be assigned after construction

    def _hydro_for(self, l):
        return self.hydro

    def fill_grav(self, name, a):
        """the Gravity_Type fill of the out-of-domain ghost zone of grav_old / grav_new (`name`)"""
        c = self.mine[0]
        if c.poisson is None:
            # monopole and constant gravity keep what the construction left there -- the monopole interpolation at the ghost
            # zone's own radius -- where the reference fills (f-row of monopole gravity: "follow-up").  Deleting
            # this return closes that follow-up.
            return
        c.hydro.grav_bc_fill(getattr(c, name), c.gravbox, c.geom)


class _Gravity:
    """What the gravity objects share: the one hierarchy they belong to (a CastroAmr, or the SingleLevel of a Castro),
    problem::center, the point mass, and the two calls of a level's advance."""
    amr = None
    center = None
    point_mass = None                           # the PointMass of the run (use_point_mass=True)

    def _belong_to(self, amr):
        if self.amr is not None and self.amr is not amr:
            raise ValueError("a %s object belongs to one Castro or one CastroAmr" % type(self).__name__)
        self.amr = amr

    def problem_center(self):
        """problem::center, resolved at every construction: this object's `center`, else the driver's `center` attribute (which
        may be assigned after construction), else the middle of the domain"""
        c = self.center if self.center is not None else getattr(self.amr, "center", None)
        if c is not None:
            return list(c)
        g = self.amr.lev[0].geom
        return [0.5 * (g.problo[d] + g.probhi[d]) for d in range(3)]

    def _add_point_mass(self, lev, name):
        """add_pointmass_to_gravity comes last (Gravity.cpp:902-907, 975-980): on top of whatever the FillPatch has put into the
        ghost zones -- on a refined level the coarse data with the coarse level's point-mass term"""
        if self.point_mass is not None and lev.mine:
            h = lev.hydro
            fabs = h.make_grav_fabs([(getattr(b, name), b.gravbox) for b in lev.mine])       # descriptors are memoised
            self.point_mass.add(h, fabs, self.problem_center(), lev.geom)

    def check_level(self, l, geom):
        pass

    def get_old_grav_vector(self, level, time=None, a=0.0):
        """grav_old of every box of `level` at the level's old time; a: where that time lies in the parent's [old, new]"""
        self._grav_vector(level, "old", time, a)

    def get_new_grav_vector(self, level, time=None, a=1.0):
        self._grav_vector(level, "new", time, a)


class ConstantGravity(_Gravity):
    """gravity.gravity_type = "ConstantGrav" as Gravity_Type data (Gravity.cpp:859-866): zero, const_grav along z, then the point
    mass (:902-907).  Made by the single-level driver for use_point_mass with constant gravity, the one case in which constant
    gravity is not one vector; CastroAmr refuses that combination."""

    def __init__(self, const_grav):
        self.const_grav = float(const_grav)

    def bind(self, amr, lo_bc, hi_bc):
        self._belong_to(amr)

    def _grav_vector(self, level, which, time, a):
        lev = self.amr.lev[level]
        name = "grav_" + which
        for b in lev.mine:
            grav = getattr(b, name)
            grav.zero_()                        # grav.setVal(0.0, ng); grav.setVal(const_grav, AMREX_SPACEDIM - 1, 1, ng)
            grav[2].fill_(self.const_grav)
        lev.fill_grav(name, a)
        self._add_point_mass(lev, name)


class MonopoleGravity(_Gravity):
    def __init__(self, drdxfac=1, Gconst=L.GCONST, center=None):
        """drdxfac: gravity.drdxfac; Gconst: the reference takes C::Gconst from its Microphysics constants (the default is the cgs
        value of that release); center: problem::center, default the driver's `center`, else the middle of the domain."""
        self.drdxfac, self.Gconst = int(drdxfac), float(Gconst)
        self.center = None if center is None else tuple(float(x) for x in center)
        if self.drdxfac < 1:
            raise ValueError("gravity.drdxfac must be at least 1, not %d" % self.drdxfac)
        self._lev = {}

    # ---- the hierarchy this object belongs to ---------------------------------------------------------------
    def bind(self, amr, lo_bc, hi_bc):
        if any(lo_bc[d] == 0 or hi_bc[d] == 0 for d in range(3)):
            if all(lo_bc[d] == 0 and hi_bc[d] == 0 for d in range(3)):
                raise ValueError("monopole gravity needs a non-periodic domain: a fully periodic one has no isolated mass to take "
                                 "the radial profile of")
            if not isinstance(amr, SingleLevel):        # a SingleLevel makes no Gravity_Type FillPatch (SingleLevel.fill_grav)
                raise NotImplementedError("monopole gravity on a partly periodic domain: the Gravity_Type FillPatch across a "
                                          "periodic boundary is not built")
        self._belong_to(amr)

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
        """the level's old / new time by default.  The reference bins the State_Type data, not Sborder: at the old-time point
        S_old_b, whose valid zones are the cleaned old state (the FillPatch only adds ghost zones around them), at the new-time
        point S_new_b after the hydro update and its clean_state."""
        lev = self.amr.lev[level]
        if time is None and level > 0:                  # the time the coarser levels are binned at; level 0 has none below it
            time = getattr(lev, "t_" + which)
        self.make_radial_gravity(level, time, which)
        ent, mono = self._arrays(level), self.params(level)
        ent["last"] = which
        name = "grav_" + which
        for b in lev.mine:
            lev.hydro.monopole_grav(ent[which], mono, lev.geom, getattr(b, name), b.gravbox)
        lev.fill_grav(name, a)
        self._add_point_mass(lev, name)

    def radial_gravity(self, level):
        """(radial_mass_summed, radial_vol_summed, radial_grav_old, radial_grav_new) of `level` after its last construction
        (_arrays(level)["last"]: "old" | "new"), numpy"""
        ent, n = self._arrays(level), self.n1d(level)
        mv = ent.get("last_summed", ent["mv"]).cpu().numpy()
        return mv[:n].copy(), mv[n:].copy(), ent["old"].cpu().numpy().copy(), ent["new"].cpu().numpy().copy()


def refuse_for_poisson(who, comm, base_grid, use_point_mass, check_int, ext_bc, geom):
    """What Poisson gravity is not built for, asked by both drivers before anything is made.  who: "" | "CastroAmr: ";
    geom: the geometry of level 0."""
    if comm is not None and comm.size > 1:
        raise NotImplementedError("%sPoisson gravity on more than one rank: the multigrid needs a halo exchange of phi on every "
                                  "level and the moments a sum over the ranks -- a follow-up" % who)
    if base_grid is not None and tuple(base_grid) != (1, 1, 1):
        raise NotImplementedError("%sPoisson gravity with base_grid: level 0 must be one box -- the multigrid has no halo exchange "
                                  "of phi between boxes; a follow-up" % who)
    if use_point_mass:
        raise NotImplementedError("%suse_point_mass with Poisson gravity (the point mass is excluded from the right-hand side "
                                  "and added to the solution) is a follow-up" % who)
    if int(check_int) > 0:
        raise NotImplementedError("%scheck_int with Poisson gravity: a bit-faithful restart needs phi of every level, the solver's "
                                  "starting guess, in the checkpoint (the reference's SD_1) -- a follow-up" % who)
    if ext_bc is not None and L.ext_bc_hse_faces(ext_bc, geom):
        raise ValueError("HSE boundaries assume constant gravity: not with PoissonGravity(...)")
    for d in range(3):
        for bc in (geom.lo_bc[d], geom.hi_bc[d]):
            if bc == 0 or bc == 3:
                raise NotImplementedError("Poisson gravity with a %s face: the mass offset of a periodic domain and the "
                                          "reflected moments / Neumann faces of a Symmetry one are a follow-up; all six faces "
                                          "must be Dirichlet faces of the potential" % ("periodic" if bc == 0 else "Symmetry"))
    lo, hi = tuple(geom.domlo[d] for d in range(3)), tuple(geom.domhi[d] for d in range(3))
    PoissonGravity._check_bottom(0, (lo, hi), tuple(hi[d] - lo[d] + 1 for d in range(3)))


class PoissonGravity(_Gravity):
    """gravity.gravity_type = "PoissonGrav": castro_amd.Castro(do_grav=True, poisson=PoissonGravity(...)) on a single level,
    castro_amd.CastroAmr(do_grav=True, gravity=PoissonGravity(..., max_solve_level=None)) on a hierarchy -- one path: the single
    level is level 0 of a hierarchy of one (SingleLevel).

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

    On a hierarchy the levels solve for themselves.  max_solve_level: gravity.max_solve_level, the finest level that solves (None:
    every level, the reference's default); a finer level takes phi and g from the level below by interpolation.  no_sync / no_composite:
    gravity.no_sync / gravity.no_composite; only True is built (no composite solve, no gravity_sync, no composite correction).
    One rank, refinement ratio 2, level 0 ONE box, every refined box inside the domain.  A refined level is one box or several
    (patches=[[box, ...]], refine= with cluster=True): a level of several boxes is solved as ONE array over their bounding box
    with a coverage mask (BOXES_OPERATIONS of the backend: castro_amd_poisson_boxes_*) -- the coarsened boxes, grown by one zone,
    must lie inside the boxes of the level below, and the level coarsens only while every box does (ValueError names the level,
    the bounding box and the alignment when the coarsest level would hold more than CASTRO_AMD_POISSON_MAX_BOTTOM zones)."""

    OPERATIONS = ("multipole_moments_mf", "multipole_phi_bc", "poisson_solve", "grad_phi_to_grav")
    AMR_OPERATIONS = ("poisson_cf_bc", "lincomb", "cc_interp")
    # a refined level of several boxes: one array over their bounding box (a backend without them keeps the refusal of such levels)
    BOXES_OPERATIONS = ("poisson_boxes_plan_create", "poisson_boxes_cf_bc", "poisson_boxes_solve", "grad_phi_to_grav_boxes")
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

    def bind(self, amr, lo_bc=None, hi_bc=None):
        """the call the other gravity objects answer too; the faces are among the checks of refuse_for_poisson"""
        self._belong_to(amr)

    plan = property(lambda self: self._lev.get(0, {}).get("plan"), doc="the multigrid plan of level 0, None when there is none")

    def close(self):
        for ent in self._lev.values():          # phi stays, a later solve makes the plan again
            self._free_plan(ent)

    @staticmethod
    def _free_plan(ent):
        if ent.get("plan") is not None:
            ent["hydro"].poisson_plan_destroy(ent["plan"])
        ent["plan"] = None

    def plan_level(self, l):
        """the multigrid plan of level l, made if there is none: construction of a Castro, the first solve, or after close()"""
        ent = self._entry(l)
        if ent["plan"] is None:
            if ent["boxes"] is None:
                ent["plan"] = ent["hydro"].poisson_plan_create(ent["geom"])
            else:
                ent["plan"] = ent["hydro"].poisson_boxes_plan_create([ent["geom"].dx[d] for d in range(3)], ent["boxes"])
        return ent["plan"]

    def __del__(self):
        try:
            # a finaliser that runs in the middle of a stream capture must not free device memory (HipHydro.__del__)
            import torch
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                return
            self.close()
        except Exception:
            pass

    # ---- level solves (gravity.no_sync = 1, gravity.no_composite = 1) ---------------------------------------------------------
    # Castro::construct_old_gravity / construct_new_gravity (Castro_gravity.cpp:14-232) and Gravity::solve_for_phi /
    # get_old_grav_vector / get_new_grav_vector / GetCrsePhi (Gravity.cpp:418-485, 664-690, 838-981) on a hierarchy whose levels
    # are one box each (a level of several boxes: the same sequence on its level array, ent["boxes"]).  Level 0 takes its boundary values from the multipole moments of its own valid zones.  A level
    # 0 < l <= max_solve_level solves on its own box
    # -- a geometry whose domain is the box goes to the same entry points -- with Dirichlet data from the potential of the level
    # below at its own time (castro_amd_poisson_cf_bc_fab).  A level above max_solve_level takes phi and g of its whole FABs from
    # the level below (FillCoarsePatch: lincomb in time, cc_interp in space).
    def solves(self, level):
        return self.max_solve_level is None or level <= self.max_solve_level

    def check_level(self, l, geom):
        """the operations a level needs of its backend; a SingleLevel never has a refined level"""
        h = self.amr._hydro_for(l)
        needed = self.OPERATIONS + (() if isinstance(self.amr, SingleLevel) else self.AMR_OPERATIONS)
        missing = [name for name in needed + ("poisson_plan_create", "grav_bc_fill") if not hasattr(h, name)]
        if missing:
            raise NotImplementedError("Poisson gravity: this backend has no %s; there is no host fallback" % ", ".join(missing))

    @staticmethod
    def _check_bottom(l, box, n):
        coarsest = L.poisson_level_extents(n)[-1]
        if coarsest[0] * coarsest[1] * coarsest[2] > L.POISSON_MAX_BOTTOM:
            raise ValueError("Poisson gravity: the box %s of level %d with n_cell = %s coarsens to %s, more than the %d zones the "
                             "bottom solver of the multigrid takes (CASTRO_AMD_POISSON_MAX_BOTTOM): its extents need more factors "
                             "of 2 -- a blocking_factor of 16 or 32" % (box, l, n, coarsest, L.POISSON_MAX_BOTTOM))

    @staticmethod
    def _check_bottom_boxes(l, boxes):
        lev = L.poisson_boxes_levels(boxes)
        (clo, cn), (lo, n) = lev[-1], lev[0]
        if cn[0] * cn[1] * cn[2] > L.POISSON_MAX_BOTTOM:
            bb = (lo, tuple(lo[d] + n[d] - 1 for d in range(3)))
            raise ValueError("Poisson gravity: the %d boxes of level %d with the bounding box %s (%s zones), aligned to %d zones, "
                             "coarsen to %s, more than the %d zones the bottom solver of the multigrid takes "
                             "(CASTRO_AMD_POISSON_MAX_BOTTOM): the level coarsens only while every box coarsens -- a larger "
                             "blocking_factor aligns the boxes to more factors of 2"
                             % (len(boxes), l, bb, n, L.poisson_boxes_alignment(boxes), cn, L.POISSON_MAX_BOTTOM))

    @staticmethod
    def _inside_union(box, parents):
        """does the box (lo, hi) lie inside the union of the boxes `parents`?"""
        import numpy as np
        lo, hi = box
        cov = np.zeros(tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0)), dtype=bool)
        for plo, phi in parents:
            a = [max(plo[d], lo[d]) - lo[d] for d in range(3)]
            b = [min(phi[d], hi[d]) - lo[d] + 1 for d in range(3)]
            if all(b[d] > a[d] for d in range(3)):
                cov[a[2]:b[2], a[1]:b[1], a[0]:b[0]] = True
        return bool(cov.all())

    def check_boxes(self, l, boxes, parents):
        """the boxes (lo, hi) of the refined level l about to be made, in its own zones; parents: those of level l - 1.  A level
        of several boxes, or over several parents, needs the operations of a level array (BOXES_OPERATIONS) of its backend."""
        several = len(boxes) != 1 or len(parents) != 1
        if len(boxes) != 1:
            h = self.amr._hydro_for(l)
            missing = [name for name in self.BOXES_OPERATIONS if not hasattr(h, name)]
            if missing:
                raise NotImplementedError("Poisson gravity: level %d would have %d boxes (level %d has %d) -- this backend has no "
                                          "%s: a level of several boxes is solved as one array over its bounding box, with a "
                                          "coverage mask" % (l, len(boxes), l - 1, len(parents), ", ".join(missing)))
        dom = tuple((2 ** l) * x for x in self.amr.n_cell)
        for lo, hi in boxes:
            if any(lo[d] <= 0 or hi[d] >= dom[d] - 1 for d in range(3)):
                raise NotImplementedError("Poisson gravity: the box %s of level %d touches the domain boundary -- the multipole "
                                          "boundary values of a refined level are not built; the box must lie inside the domain"
                                          % ((lo, hi), l))
        if not several:
            if not self.solves(l):
                return
            (lo, hi), (plo, phi) = boxes[0], parents[0]
            if any((lo[d] >> 1) - 1 < plo[d] or (hi[d] >> 1) + 1 > phi[d] for d in range(3)):
                raise ValueError("Poisson gravity: the box %s of level %d, coarsened and grown by one zone, does not lie inside the "
                                 "valid box %s of level %d: its boundary values would read ghost zones of the coarse potential"
                                 % ((lo, hi), l, (plo, phi), l - 1))
            self._check_bottom(l, (lo, hi), tuple(hi[d] - lo[d] + 1 for d in range(3)))
            return
        # the coarse zones the boundary values and the interpolated guess read (edges included: the transverse slopes) must be
        # valid zones of level l - 1: an uncovered or ghost zone of the coarse potential is never read
        for lo, hi in boxes:
            need = (tuple((x >> 1) - 1 for x in lo), tuple((x >> 1) + 1 for x in hi))
            if not self._inside_union(need, parents):
                raise ValueError("Poisson gravity: the box %s of level %d, coarsened and grown by one zone, does not lie inside the "
                                 "union of the %d boxes of level %d: its boundary values would read zones of the coarse potential "
                                 "that level %d does not cover" % ((lo, hi), l, len(parents), l - 1, l - 1))
        if not self.solves(l):
            return
        if len(boxes) == 1:
            self._check_bottom(l, boxes[0], tuple(boxes[0][1][d] - boxes[0][0][d] + 1 for d in range(3)))
        else:
            self._check_bottom_boxes(l, boxes)

    def reset(self, from_level=0):
        """regrid / _push_level / _drop_fine: the levels >= from_level are gone or re-made -- their potentials and plans go"""
        for l in list(self._lev):
            if l >= from_level:
                self._free_plan(self._lev[l])
                del self._lev[l]

    def _entry(self, l):
        """phi_old / phi_new (one ghost zone), the plan and the scratch of level l, made for the box the level has now -- for the
        boxes: a level of several is ONE array over their bounding box, with three face-centred arrays for its boundary values"""
        lev = self.amr.lev[l]
        b = lev.mine[0]
        boxes = tuple(x.bx for x in lev.mine) if len(lev.mine) > 1 else None
        key = b.bx if boxes is None else boxes
        ent = self._lev.get(l)
        if ent is not None and ent["key"] != key:        # a plan is kept per level, keyed by the extents of its box(es)
            self._free_plan(ent)
            ent = None
        if ent is None:
            h = lev.hydro
            bb = b.bx if boxes is None else (tuple(min(x[0][d] for x in boxes) for d in range(3)),
                                             tuple(max(x[1][d] for x in boxes) for d in range(3)))
            phibox = (tuple(x - 1 for x in bb[0]), tuple(x + 1 for x in bb[1]))
            ent = self._lev[l] = dict(key=key, hydro=h, phibox=phibox, phi_old=h.alloc(1, *phibox), phi_new=h.alloc(1, *phibox),
                                      plan=None, have=(l == 0), tables={}, stats={"first": None, "old": None, "new": None},
                                      boxes=boxes, bb=bb)
            if boxes is not None:
                ent["geom"] = lev.geom
                ent["facebox"] = (bb[0], tuple(x + 1 for x in bb[1]))
                ent["faces"] = h.alloc(3, *ent["facebox"])
                ent["cbox"] = (tuple((x >> 1) - 2 for x in bb[0]), tuple((x >> 1) + 2 for x in bb[1]))
                ent["ctmp"] = h.alloc(1, *ent["cbox"])
            elif l == 0:
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

    def _grav_vector(self, level, which, time, a):
        """phi and g of `level` at its old / new time (`time` itself is not read: a level solves from its own state)"""
        import math
        lev = self.amr.lev[level]
        b = lev.mine[0]
        h = lev.hydro
        ent = self._entry(level)
        name = "grav_" + which
        grav = getattr(b, name)
        phi, pbx = ent["phi_" + which], ent["phibox"]
        boxes = ent["boxes"]
        if level > 0 and not self.solves(level):
            # no solve above max_solve_level: phi and g of the whole FABs are the FillCoarsePatch of the level below
            # (Gravity.cpp:466, 846-852, 919-925); on a level of several boxes, box by box -- phi on the valid zones of each
            self._crse_at(level, ent, a)
            if boxes is None:
                h.cc_interp(ent["ctmp"], ent["cbox"], phi, pbx, pbx[0], pbx[1], 1)
            ent["have"] = True
            for x in lev.mine:
                if boxes is not None:
                    h.cc_interp(ent["ctmp"], ent["cbox"], phi, pbx, x.lo, x.hi, 1)
                for p, (lo, hi) in x.gsrc + x.gsrc_valid:
                    h.lincomb(x.gctmp, x.gcbox, 1.0 - a, p.grav_old, p.gravbox, a, p.grav_new, p.gravbox, 3, lo, hi)
                h.cc_interp(x.gctmp, x.gcbox, getattr(x, name), x.gravbox, x.gravbox[0], x.gravbox[1], 3)
            return
        if not ent["have"]:
            # the first solve of the level, or of a level a regrid has re-made: the level below, interpolated, is the guess
            self._crse_at(level, ent, a)
            for x in lev.mine:
                h.cc_interp(ent["ctmp"], ent["cbox"], phi, pbx, x.lo, x.hi, 1)
            ent["have"] = True
        elif which == "new":
            phi.copy_(ent["phi_old"])                    # the "old" phi of the step is the guess (Castro_gravity.cpp:146)
        plan = self.plan_level(level)
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
        elif boxes is None:
            P = self._lev[level - 1]
            h.poisson_cf_bc(phi, pbx, b.lo, b.hi, P["phi_old"], P["phibox"], P["phi_new"], P["phibox"], a)
        else:
            P = self._lev[level - 1]
            h.poisson_boxes_cf_bc(plan, ent["faces"], ent["facebox"], P["phi_old"], P["phibox"], P["phi_new"], P["phibox"], a)
        if boxes is None:
            cycles, ok, norm, hist = h.poisson_solve(plan, phi, pbx, S, b.gbox, L.URHO, 4.0 * math.pi * self.Gconst,
                                                     self.reltol, self.abstol, self.maxiter)
        else:
            rhos = [(x.S_old_b if which == "old" else x.S_new_b, x.gbox) for x in lev.mine]
            cycles, ok, norm, hist = h.poisson_boxes_solve(plan, phi, pbx, ent["faces"], ent["facebox"], rhos, L.URHO,
                                                           4.0 * math.pi * self.Gconst, self.reltol, self.abstol, self.maxiter)
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
        if boxes is None:
            h.grad_phi_to_grav(phi, pbx, grav, b.gravbox, ent["geom"])
        else:
            h.grad_phi_to_grav_boxes(plan, phi, pbx, ent["faces"], ent["facebox"], [(getattr(x, name), x.gravbox) for x in lev.mine])
        lev.fill_grav(name, a)                           # the Gravity_Type FillPatch of the ghost zones of g

    def phi_level(self, level, new=True):
        ent = self._entry(level)
        if ent["boxes"] is not None:
            raise ValueError("phi_grav(%d): level %d has %d boxes and its potential is one array over their bounding box with a "
                             "coverage mask -- phi_grav_level(%d) returns it" % (level, level, len(ent["boxes"]), level))
        return ent["phi_new" if new else "phi_old"]

    def phi_level_boxes(self, level, new=True):
        """(bounding box, phi on its zones, covered) of `level` as numpy arrays (nz, ny, nx): a level of one box is all covered"""
        import numpy as np
        ent = self._entry(level)
        (lo, hi) = bb = ent["bb"]
        phi = ent["phi_new" if new else "phi_old"].cpu().numpy()[0, 1:-1, 1:-1, 1:-1].copy()
        cov = np.zeros(phi.shape, dtype=bool)
        for blo, bhi in ent["boxes"] or (bb,):
            cov[tuple(slice(blo[d] - lo[d], bhi[d] - lo[d] + 1) for d in (2, 1, 0))] = True
        return bb, phi, cov

    def stats_level(self, level):
        return dict(self._entry(level)["stats"])

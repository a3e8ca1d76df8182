"""AMR with subcycling: a coarse level covering the domain and any number of refined levels (ratio 2), each a list of
boxes.

SURVEY.md 8 f-3.  What the reference does through AMReX's Amr / AmrLevel / FluxRegister / Interpolater / grid
generation classes [3P] is orchestrated here on top of `Castro` objects, one per box:

  Amr::timeStep recursion with subcycling        coarse advance, then two fine advances of dt/2, down the hierarchy
  AmrLevel::FillPatch (fine level)               cell_cons_interp of the time-interpolated coarse state
                                                 (Castro_setup.cpp:352-364, Castro.cpp:4201-4209), clean_state of those
                                                 ghost zones (Castro_advance.cpp:186), then valid data of the other
                                                 boxes of the level, then the physical boundary fill
  Castro::FluxRegCrseInit / FluxRegFineAdd       Castro.cpp:2487-2545 -- one register per face of every fine box
  Castro::post_timestep: reflux, avgDown,        Castro.cpp:2549-2700, 3096-3113, post_timestep (:2140-2260); a coarse
      clean_state                                zone under another fine box is refluxed too and then overwritten by
                                                 avgDown, like in AMReX
  Castro::computeNewDt / computeInitialDt        Castro.cpp:1629-1866 over all levels (n_cycle = 1, 2, 2, ...)
  Castro::errorEst + Amr::regrid / grid_places   amr.refinement_indicators (AMRErrorTag [3P] restated) on every level
                                                 below max_level, whenever a level has taken regrid_int steps since
                                                 its last regrid (Amr::level_count; grids above it): tags from the finest
                                                 level down, buffered by n_error_buf, united with the (coarsened,
                                                 buffered) new boxes of the level above (proper nesting), clustered
                                                 into boxes (castro_amd/cluster.py: Berger-Rigoutsos with grid_eff,
                                                 blocking_factor, max_grid_size; `cluster=False`: one bounding box per
                                                 level).  New boxes take the data of the old boxes of their level
                                                 where they overlap and interpolated coarse data elsewhere; a regrid
                                                 adds at most one level; Amr::bldFineLevels at start-up.

Fixed hierarchies: `patches=[...]`, one entry per refined level: a box (lo, hi) or a list of boxes, in the zones of
the level below.  Level 0 is one box (per rank; this driver is single-rank).
Periodic domains: the periodic images of the boxes of a level enter the same-level copies and the reflux as boxes shifted
by the domain extent.  Constant gravity and rotation sources on every level (the Source_Type FillPatch of a refined level
interpolates the coarse sources like the state); monopole self-gravity with gravity=MonopoleGravity(...) (castro_amd/gravity.py:
the radial arrays span the levels, _Level.fill_grav is the Gravity_Type FillPatch); tracer particles with
tracers=TracerParticles(...) (castro_amd/particles.py: advected at the end of every level's advance, redistributed and
timestamped at the end of its post_timestep and after every regrid).  Not provided: multi-rank AMR.  The interpolation,
flux-register and clustering arithmetic is AMReX's, restated from its published description
(include/castro_hydro_amd.h, castro_amd/cluster.py): parity with an AMReX build is unpinned.
"""
import itertools
import os

import numpy as np
import torch

from . import _lib as L
from . import cluster as CL
from .castro import Castro, NUM_GROW, NUM_STATE, checked_estimate, density_failure, shell_slabs
from .checkpoint import CheckpointMixin

NSRC = 7                     # components of Source_Type (Castro_setup.cpp:317-327)


def _coarsen(i):
    return i // 2            # floor division is AMReX's coarsen() for negative indices too


def _shift(box, sh):
    """The box (lo, hi) moved by sh zones.  A FAB described with a shifted box is read at index - sh: this is how the
    periodic images of a box enter the same-index copy / reflux operations without any kernel knowing about them."""
    return tuple(box[0][d] + sh[d] for d in range(3)), tuple(box[1][d] + sh[d] for d in range(3))


def _box_minus(box, cut):
    """The box minus the box `cut` as a list of boxes (shell_slabs around the part of `cut` that lies inside it)."""
    it = CL.intersect(box, cut)
    if not it:
        return [box]
    return [sl for sl in shell_slabs(box, it) if all(sl[1][d] >= sl[0][d] for d in range(3))]


def _is_box(x):
    return len(x) == 2 and len(x[0]) == 3 and not hasattr(x[0][0], "__len__")


class _Patch(Castro):
    """One box of a refined level: FillPatch takes ghost zones from the coarser level and from its siblings."""

    def bind(self, level, pbox):
        self.level, self.pbox = level, pbox
        if pbox is None:                       # a box of a level-0 that is cut into several boxes: nothing coarser
            self.cbox, self.ctmp, self.shell, self.regs = None, None, [], {}
            if self.have_sources:
                self.new_source_g = self.hydro.alloc(NSRC, *self.sbox) if self.owned else None
            if self.monopole:
                self.gcbox, self.gctmp, self.gshell = None, None, []
            return
        # coarse zones under the grown fine box, grown by one for the slopes
        self.cbox = (tuple(_coarsen(self.glo[d]) - 1 for d in range(3)), tuple(_coarsen(self.ghi[d]) + 1 for d in range(3)))
        self.ctmp = self.hydro.alloc(NUM_STATE, *self.cbox) if self.owned else None
        self.shell = shell_slabs(self.gbox, self.bx)
        if self.have_sources:
            self._bind_sources()
        if self.monopole:
            self._bind_gravity()
        # flux registers: the coarse faces on the six sides of this box
        plo, phi = pbox
        self.regs = {}
        for d in range(3):
            for side in (0, 1):
                rlo, rhi = list(plo), list(phi)
                rlo[d] = rhi[d] = (plo[d] if side == 0 else phi[d] + 1)
                self.regs[(d, side)] = (self.hydro.alloc(NUM_STATE, rlo, rhi) if self.owned else None, (tuple(rlo), tuple(rhi)))

    def _bind_sources(self):
        """Source_Type data (NUM_GROW_SRC ghost zones): the coarse zones under the grown box, and the ghost shell."""
        slo, shi = self.sbox
        self.scbox = (tuple(_coarsen(slo[d]) - 1 for d in range(3)), tuple(_coarsen(shi[d]) + 1 for d in range(3)))
        self.stmp = self.hydro.alloc(NSRC, *self.scbox) if self.owned else None
        self.new_source_g = self.hydro.alloc(NSRC, *self.sbox) if self.owned else None
        self.sshell = shell_slabs(self.sbox, self.bx)

    def _bind_gravity(self):
        """Gravity_Type data (one ghost zone): the ghost shell inside the domain -- the zones outside it get the boundary fill --
        and the coarse zones under it, grown by one for the slopes."""
        g = self.geom
        ilo = tuple(max(self.gravbox[0][d], g.domlo[d]) for d in range(3))
        ihi = tuple(min(self.gravbox[1][d], g.domhi[d]) for d in range(3))
        self.gcbox = (tuple(_coarsen(ilo[d]) - 1 for d in range(3)), tuple(_coarsen(ihi[d]) + 1 for d in range(3)))
        self.gctmp = self.hydro.alloc(3, *self.gcbox) if self.owned else None
        self.gshell = [sl for sl in shell_slabs((ilo, ihi), self.bx) if all(sl[1][d] >= sl[0][d] for d in range(3))]

    def expand_state(self, S, box=None, neighbors=None):
        assert box is None, "the Source_Type FillPatch of a refined level is level-wide: _Level.fill_source"
        self.level.fill_box(self, S)


class _Level:
    """The boxes of one level and the level-wide parts of Castro::advance."""

    def __init__(self, amr, l, boxes):
        self.amr, self.l, self.boxes = amr, l, list(boxes)
        self.mine = [b for b in self.boxes if b.owned]        # the boxes this rank advances (all of them on one rank)
        self.alpha = 0.0          # (t_level - t_parent_old) / dt_parent of the FillPatch being prepared
        b0 = self.boxes[0]
        self.hydro, self.params, self.geom = b0.hydro, b0.params, b0.geom
        self.red = self.mine[0].red if self.mine else self.hydro.alloc(1, (0, 0, 0), (2, 0, 0)).reshape(3)
        for b in self.mine:
            b.red = self.red      # one [min dt, min rho] pair for the level: every box reduces into it
            if b.ext_bc is not None:       # and one count of unconverged HSE columns behind it
                b._red_all, b._unconverged = self.mine[0]._red_all, self.mine[0]._unconverged
            b.fuse_post_clean = False      # post_timestep's clean_state comes after reflux and avgDown (_time_step)
        self._pending_cleans, self._post_clean_done, self._whole_step = 2, False, False
        for k in ("use_retry", "retry_subcycle_factor", "max_subcycles", "dt_cutoff", "max_dt", "fixed_dt", "have_sources"):
            setattr(self, k, getattr(b0, k))
        self.fuse_clean = b0.fuse_clean
        self.nsubcycles, self.nretries, self.last_failure = 0, 0, ""
        self.time, self.nstep = 0.0, 0
        # castro.source_term_predictor: Castro::lastDt of this level (1e200 in every constructor, Castro.cpp:906 -- a level made
        # by a regrid starts with it again) and the in_retry flag of subcycle_advance_ctu
        self.lastDt, self._in_retry = 1.e200, False
        self._iteration = 1       # Amr::timeStep's iteration of the advance in progress (1 on level 0, 1 or 2 above)
        if getattr(amr, "tracers", None) is not None:
            for b in self.mine:   # the half-time state the tracer velocity is gathered from
                b.S_half_b = b.hydro.alloc(NUM_STATE, b.glo, b.ghi)

    def __getattr__(self, name):
        # a level of one box answers for its box (S_new(), lo, hi, n, gbox, S_new_b, ...)
        boxes = self.__dict__.get("boxes", ())
        if len(boxes) == 1 and boxes[0].owned:
            return getattr(boxes[0], name)
        raise AttributeError("%s (level %d has %d boxes)" % (name, self.__dict__.get("l", -1), len(boxes)))

    def box_list(self):
        return [b.bx for b in self.boxes]

    # ---- static overlap tables (rebuilt at every regrid) -----------------------------------------
    def bind(self):
        self.plain_base = self.l == 0 and len(self.boxes) == 1 and not isinstance(self.boxes[0], _Patch)
        if self.plain_base:                    # the whole domain in one Castro box: it fills its own ghost zones
            return
        parents = self.amr.lev[self.l - 1].boxes if self.l > 0 else []
        # periodic images: shifts by the domain extent (in zones of this level / of the parent level)
        per = self.amr.periodic
        ext = [(2 ** self.l) * self.amr.n_cell[d] for d in range(3)]
        shifts = list(itertools.product(*[(-ext[d], 0, ext[d]) if per[d] else (0,) for d in range(3)]))
        cshifts = [tuple(x // 2 for x in sh) for sh in shifts]
        for b in self.boxes:
            b.sib = [(s, it, sh) for s in self.boxes for sh in shifts if not (s is b and sh == (0, 0, 0))
                     for it in [CL.intersect(b.gbox, _shift(s.bx, sh))] if it]
            b.at_domain_edge = any(b.glo[d] < b.geom.domlo[d] or b.ghi[d] > b.geom.domhi[d] for d in range(3))
            if self.have_sources:                                # the same table for the Source_Type FillPatch
                b.ssib = [(sb, it, sh) for sb in self.boxes for sh in shifts if not (sb is b and sh == (0, 0, 0))
                          for it in [CL.intersect(b.sbox, _shift(sb.bx, sh))] if it]
            if b.monopole:                                       # the same table for the Gravity_Type FillPatch (one ghost zone)
                b.gsib = [(sb, it, sh) for sb in self.boxes for sh in shifts if not (sb is b and sh == (0, 0, 0))
                          for it in [CL.intersect(b.gravbox, _shift(sb.bx, sh))] if it]
                b.grav_at_edge = any(b.gravbox[0][d] < b.geom.domlo[d] or b.gravbox[1][d] > b.geom.domhi[d] for d in range(3))
                b.gsrc = [(p, it) for p in parents for it in [CL.intersect(b.gcbox, p.gravbox)] if it] if self.l > 0 else []
                b.gsrc_valid = [(p, it) for p in parents for it in [CL.intersect(b.gcbox, p.bx)] if it] if self.l > 0 else []
                if self.l > 0:
                    cov = np.zeros(tuple(b.gcbox[1][d] - b.gcbox[0][d] + 1 for d in (2, 1, 0)), dtype=bool)
                    o = b.gcbox[0]
                    for _, (lo, hi) in b.gsrc:
                        cov[lo[2] - o[2]:hi[2] - o[2] + 1, lo[1] - o[1]:hi[1] - o[1] + 1, lo[0] - o[0]:hi[0] - o[0] + 1] = True
                    assert cov.all(), "box %s of level %d not properly nested: the coarse zones under its gravity ghost zones " \
                        "reach beyond the gravity data of level %d" % (b.bx, self.l, self.l - 1)
            if self.l == 0:                    # no coarser level: no coarse data, no flux registers, nothing to average onto
                b.csrc, b.csrc_valid, b.crse_init, b.reflux_to, b.flux_to, b.avg_to = [], [], {}, {}, {}, []
                if self.have_sources:
                    b.ssrc, b.ssrc_valid, b.sshell = [], [], []
                continue
            b.csrc = [(p, it) for p in parents for it in [CL.intersect(b.cbox, p.gbox)] if it]
            if len(b.csrc) == 1:
                assert b.csrc[0][1] == b.cbox, "box not properly nested: its ghost zones need parent data beyond the parent's own ghost zones"
                b.csrc_valid = []
            else:
                # several parents: ghost zones first, valid zones last, so that valid data wins
                b.csrc_valid = [(p, it) for p in parents for it in [CL.intersect(b.cbox, p.bx)] if it]
                cov = np.zeros(tuple(b.cbox[1][d] - b.cbox[0][d] + 1 for d in (2, 1, 0)), dtype=bool)
                for _, (lo, hi) in b.csrc:
                    o = b.cbox[0]
                    cov[lo[2] - o[2]:hi[2] - o[2] + 1, lo[1] - o[1]:hi[1] - o[1] + 1, lo[0] - o[0]:hi[0] - o[0] + 1] = True
                assert cov.all(), "box not properly nested in the union of its parents"
            # FluxRegCrseInit sources and reflux targets per register
            b.crse_init, b.reflux_to, b.flux_to = {}, {}, {}
            for (d, side), (reg, rbox) in b.regs.items():
                b.crse_init[(d, side)] = [(p, it) for p in parents for it in [CL.intersect(rbox, p.flux_boxes[d])] if it]
                sh = -1 if side == 0 else 0           # the coarse zone outside the fine box: face - 1 (low side) or face
                zlo, zhi = list(rbox[0]), list(rbox[1])
                zlo[d] += sh; zhi[d] += sh
                tg = []
                for p in parents:
                    for csh in cshifts:                  # a coarse zone beyond a periodic boundary is its image inside
                        it = CL.intersect((tuple(zlo), tuple(zhi)), _shift(p.bx, csh))
                        if it:
                            flo, fhi = list(it[0]), list(it[1])
                            flo[d] -= sh; fhi[d] -= sh
                            tg.append((p, (tuple(flo), tuple(fhi)), csh))
                b.reflux_to[(d, side)] = tg
                # the faces of this register on the coarse-fine boundary (FluxRegister::ClearInternalBorders [3P]: a face that is
                # also a face of the opposite side of a box of this level, or of a periodic image of one, lies between two fine
                # boxes) and the parents' flux FABs that hold them -- a face on the seam of two parents is in both, a face beyond
                # a periodic boundary is its image inside: castro.update_sources_after_reflux (Castro.cpp:2617-2644)
                faces = [rbox]
                for s2 in self.boxes:
                    for csh in cshifts:
                        cut = _shift(s2.regs[(d, 1 - side)][1], csh)
                        faces = [x for f in faces for x in _box_minus(f, cut)]
                b.flux_to[(d, side)] = [(p, it, csh) for f in faces for p in parents for csh in cshifts
                                        for it in [CL.intersect(f, _shift(p.flux_boxes[d], csh))] if it]
                # proper nesting (AMReX's Amr::grid_places guarantees it): every parent-level zone next to a face of
                # this box is a valid zone of the parent level (or lies outside a non-periodic domain); a face that
                # touched a still coarser level directly would lose its flux correction
                cdom = [(2 ** (self.l - 1)) * self.amr.n_cell[x] for x in range(3)]
                if not per[d]:
                    zlo[d], zhi[d] = max(zlo[d], 0), min(zhi[d], cdom[d] - 1)
                want = int(np.prod([max(zhi[x] - zlo[x] + 1, 0) for x in range(3)]))
                have = sum(int(np.prod([fhi[x] - flo[x] + 1 for x in range(3)])) for _, (flo, fhi), _ in tg)
                assert have == want, "box %s of level %d not properly nested: zones of level %d next to its %s face " \
                    "belong to no box of that level" % (b.bx, self.l, self.l - 1, "xyz"[d] + "-+"[side])
            b.avg_to = [(p, it) for p in parents for it in [CL.intersect(b.pbox, p.bx)] if it]
            if self.have_sources:                                # the same tables for the Source_Type FillPatch
                b.ssrc = [(p, it) for p in parents for it in [CL.intersect(b.scbox, p.sbox)] if it]
                b.ssrc_valid = [(p, it) for p in parents for it in [CL.intersect(b.scbox, p.bx)] if it]
        self._op_cache = {}
        self.batched = hasattr(self.hydro, "make_ops") and self.amr.nranks == 1
        if self.batched and self.l > 0:
            # flux-register operations never change between regrids (registers and flux FABs keep their storage)
            mk = self.hydro.make_ops
            self.ops_fine_add = mk([(L.OP_FLUXREG_FINE_ADD, d, NUM_STATE, rbox[0], rbox[1], 1.0, 0.0, (reg, rbox),
                                     (b.fluxes[d], b.flux_boxes[d]), None)
                                    for b in self.boxes for (d, side), (reg, rbox) in b.regs.items()])
            self.ops_crse_init = mk([(L.OP_FLUXREG_CRSE_INIT, d, NUM_STATE, lo, hi, -1.0, 0.0, (reg, rbox),
                                      (p.fluxes[d], p.flux_boxes[d]), None)
                                     for b in self.boxes for (d, side), (reg, rbox) in b.regs.items()
                                     for p, (lo, hi) in b.crse_init[(d, side)]])

    # ---- AmrLevel::FillPatch ---------------------------------------------------------------------
    def _interp_ghosts(self, b, S):
        h, a = self.hydro, self.alpha
        # StateData time interpolation of the coarse data: (1 - a) old + a new
        for p, (lo, hi) in b.csrc + b.csrc_valid:
            h.lincomb(b.ctmp, b.cbox, 1.0 - a, p.S_old_b, p.gbox, a, p.S_new_b, p.gbox, NUM_STATE, lo, hi)
        if hasattr(h, "fillpatch_shell"):                       # both passes over the six slabs in one launch
            h.fillpatch_shell(b.ctmp, b.cbox, S, b.gbox, b.lo, b.hi, NUM_GROW, b.params, ntimes=1)
            return
        self._interp_shell(b, S)

    def _copy_siblings(self, b, S, which):
        h = self.hydro
        for s, (lo, hi), sh in b.sib:
            h.copy(S, b.gbox, getattr(s, which), _shift(s.gbox, sh), lo, hi)
        self._bc_fill_state(b, S)                              # fine zones outside the domain

    def _bc_fill_state(self, b, S):
        """the physical-boundary fill of a state array of box b: the generic fill, then -- with ext_bc -- the ambient and
        hydrostatic overrides (Castro._bc_fill_state on the level's context)"""
        self.hydro.bc_fill(S, b.gbox, b.geom)
        if b.ext_bc is not None:
            self.hydro.ext_bc_fill(S, b.gbox, b.geom, b.params, b.ext_bc, unconverged=b._unconverged)

    def _read_red(self):
        """self.red on the host; with ext_bc the same copy carries the count of unconverged HSE columns (Castro._read_red)"""
        if self.mine and self.mine[0].ext_bc is not None:
            return self.mine[0]._read_red()
        return self.red.tolist()

    def _cached_ops(self, key, ptrs, build):
        """Operation tables hold raw pointers: S_old_b / S_new_b swap at every advance, so a table is kept per
        pointer configuration (two in the steady state)."""
        ent = self._op_cache.get((key, ptrs))
        if ent is None:
            if len(self._op_cache) > 256:
                self._op_cache.clear()
            ent = build()
            self._op_cache[(key, ptrs)] = ent
        return ent

    def fill(self, which):
        """Ghost zones of S_old_b / S_new_b (`which`) of every box of the level."""
        if self.plain_base:
            for b in self.mine:
                b.expand_state(getattr(b, which))
            return
        if self.amr.nranks > 1:
            return self._fill_ranks(which)
        if not self.batched:
            for b in self.boxes:
                if self.l > 0:
                    self._interp_ghosts(b, getattr(b, which))
            for b in self.boxes:                               # valid zones are final only after every box's clean pass
                self._copy_siblings(b, getattr(b, which), which)
            return
        h, a = self.hydro, self.alpha
        parents = self.amr.lev[self.l - 1].boxes if self.l > 0 else []
        # 1. time-interpolated coarse data under every box, all boxes in a few launches.  Where a box has several parents
        #    their grown boxes overlap: the ghost-zone pass goes first (overlapping entries carry identical values: a
        #    ghost zone of one parent is a copy of the valid zone of another or the same interpolation), the valid-zone
        #    pass second, as separate launches
        pp = tuple(t.data_ptr() for p in parents for t in (p.S_old_b, p.S_new_b))
        for key, attr in ((("lincomb_ghost", "csrc"), ("lincomb_valid", "csrc_valid")) if self.l > 0 else ()):
            ops = self._cached_ops((key,), pp, lambda attr=attr: h.make_ops(
                [(L.OP_LINCOMB, 0, NUM_STATE, lo, hi, 0.0, 0.0, (b.ctmp, b.cbox), (p.S_old_b, p.gbox), (p.S_new_b, p.gbox))
                 for b in self.boxes for p, (lo, hi) in getattr(b, attr)]))
            arr, n = ops
            for i in range(n):
                arr[i].a, arr[i].b = 1.0 - a, a
            h.fab_ops(ops)
        # 2. interpolation + clean_state of the ghost shells: one launch for the level (six slab operations per box)
        if self.l > 0 and self._level_calls():
            sp2 = tuple(getattr(b, which).data_ptr() for b in self.boxes)
            h.fab_ops(self._cached_ops(("shell", which), sp2, lambda: h.make_ops(
                [(L.OP_INTERP_CLEAN, 0, NUM_STATE, lo, hi, 1.0, 0.0, (getattr(b, which), b.gbox), (b.ctmp, b.cbox), None)
                 for b in self.boxes for lo, hi in b.shell if all(hi[d] >= lo[d] for d in range(3))])), params=self.params)
        else:
            for b in (self.boxes if self.l > 0 else ()):
                h.fillpatch_shell(b.ctmp, b.cbox, getattr(b, which), b.gbox, b.lo, b.hi, NUM_GROW, b.params, ntimes=1)
        # 3. valid zones of the siblings (final only after every box's clean pass), all boxes in a few launches
        sp = tuple(getattr(b, which).data_ptr() for b in self.boxes)
        h.fab_ops(self._cached_ops(("sib", which), sp, lambda: h.make_ops(
            [(L.OP_COPY, 0, NUM_STATE, lo, hi, 0.0, 0.0, (getattr(b, which), b.gbox), (getattr(sb, which), _shift(sb.gbox, sh)), None)
             for b in self.boxes for sb, (lo, hi), sh in b.sib])))
        # 4. physical boundaries
        for b in self.boxes:
            if b.at_domain_edge:
                self._bc_fill_state(b, getattr(b, which))

    def _fill_ranks(self, which):
        """fill() with the boxes of this level and of the parent level spread over ranks: the same four passes, every
        box-to-box transfer through CastroAmr._xrun (local where both boxes are here, one message otherwise)."""
        h, a, X = self.hydro, self.alpha, self.amr._xrun
        X([("lincomb", b, p, lo, hi, a) for b in self.boxes for p, (lo, hi) in b.csrc])           # ghost zones of the parents first,
        X([("lincomb", b, p, lo, hi, a) for b in self.boxes for p, (lo, hi) in b.csrc_valid])     # valid zones last
        for b in (self.mine if self.l > 0 else ()):
            h.fillpatch_shell(b.ctmp, b.cbox, getattr(b, which), b.gbox, b.lo, b.hi, NUM_GROW, b.params, ntimes=1) \
                if hasattr(h, "fillpatch_shell") else self._interp_shell(b, getattr(b, which))
        X([("copy", b, sb, lo, hi, (which, sh)) for b in self.boxes for sb, (lo, hi), sh in b.sib])
        for b in self.mine:
            self._bc_fill_state(b, getattr(b, which))

    def _interp_shell(self, b, S):
        for lo, hi in b.shell:
            self.hydro.cc_interp(b.ctmp, b.cbox, S, b.gbox, lo, hi, NUM_STATE)
        for lo, hi in b.shell:                                 # clean_state(Sborder) reaches the ghost zones too
            self.hydro.clean_state(S, b.gbox, lo, hi, b.params, ntimes=1)

    def fill_box(self, b, S):
        which = "S_new_b" if S is b.S_new_b else "S_old_b"
        assert S is getattr(b, which)
        if self.l > 0:
            self._interp_ghosts(b, S)
        self._copy_siblings(b, S, which)

    # ---- AmrLevel::FillPatch of Source_Type (Castro_advance_ctu.cpp:138-140) ------------------------------
    def fill_source(self, name):
        """Ghost zones of the Source_Type data `name` (old_source / new_source_g) of every box: coarse Source_Type data
        interpolated in time ((1 - alpha) old + alpha new, StateData's rule) and space (cell_cons_interp,
        Castro_setup.cpp:317-327), valid data of the other boxes of the level, physical boundaries."""
        if self.plain_base:
            for b in self.mine:
                b.expand_state(getattr(b, name), b.sbox, b.src_neighbors)
            return
        h, a = self.hydro, self.alpha
        if self.amr.nranks > 1:
            X = self.amr._xrun
            X([("src_lincomb", b, p, lo, hi, a) for b in self.boxes for p, (lo, hi) in b.ssrc + b.ssrc_valid], NSRC)
            for b in self.mine:
                for lo, hi in b.sshell:
                    h.cc_interp(b.stmp, b.scbox, getattr(b, name), b.sbox, lo, hi, NSRC)
            X([("src_copy", b, sb, lo, hi, (name, sh)) for b in self.boxes for sb, (lo, hi), sh in b.ssib], NSRC)
            for b in self.mine:
                h.bc_fill(getattr(b, name), b.sbox, b.geom)
            return
        if self.batched and self._level_calls():
            # The same four passes with every box of the level in one launch each (as fill() does for the state): a level of
            # 56 boxes made ~1000 launches here per advance.  Source_Type tensors keep their storage between regrids: one table
            # per (pass, name), the time-interpolation weights rewritten per call.
            mk, P = h.make_ops, self.params
            for key, attr in ((("src_lincomb_ghost", "ssrc"), ("src_lincomb_valid", "ssrc_valid")) if self.l > 0 else ()):
                ops = self._cached_ops((key,), (), lambda attr=attr: mk(
                    [(L.OP_LINCOMB, 0, NSRC, lo, hi, 0.0, 0.0, (b.stmp, b.scbox), (p.old_source, p.sbox), (p.new_source_g, p.sbox))
                     for b in self.boxes for p, (lo, hi) in getattr(b, attr)]))
                arr, n = ops
                for i in range(n):
                    arr[i].a, arr[i].b = 1.0 - a, a
                h.fab_ops(ops, params=P)
            if self.l > 0:
                h.fab_ops(self._cached_ops(("src_shell", name), (), lambda: mk(
                    [(L.OP_INTERP, 0, NSRC, lo, hi, 0.0, 0.0, (getattr(b, name), b.sbox), (b.stmp, b.scbox), None)
                     for b in self.boxes for lo, hi in b.sshell if all(hi[d] >= lo[d] for d in range(3))])), params=P)
            h.fab_ops(self._cached_ops(("src_sib", name), (), lambda: mk(
                [(L.OP_COPY, 0, NSRC, lo, hi, 0.0, 0.0, (getattr(b, name), b.sbox), (getattr(sb, name), _shift(sb.sbox, sh)), None)
                 for b in self.boxes for sb, (lo, hi), sh in b.ssib])), params=P)
            for b in self.boxes:
                if b.at_domain_edge:
                    h.bc_fill(getattr(b, name), b.sbox, b.geom)
            return
        for b in self.boxes:
            for p, (lo, hi) in b.ssrc + b.ssrc_valid:           # ghost zones of the parents first, valid zones last
                h.lincomb(b.stmp, b.scbox, 1.0 - a, p.old_source, p.sbox, a, p.new_source_g, p.sbox, NSRC, lo, hi)
            for lo, hi in b.sshell:
                h.cc_interp(b.stmp, b.scbox, getattr(b, name), b.sbox, lo, hi, NSRC)
        for b in self.boxes:
            for sb, (lo, hi), sh in b.ssib:
                h.copy(getattr(b, name), b.sbox, getattr(sb, name), _shift(sb.sbox, sh), lo, hi)
            h.bc_fill(getattr(b, name), b.sbox, b.geom)

    def fill_new_source(self):
        """The new-time Source_Type data with ghost zones, for the FillPatch of the next finer level."""
        h = self.hydro
        for b in self.mine:
            h.copy(b.new_source_g, b.sbox, b.new_source, b.bx, b.lo, b.hi)
        self.fill_source("new_source_g")

    # ---- AmrLevel::FillPatch of Gravity_Type (Gravity.cpp:894-900, 967-973) ------------------------------------
    def fill_grav(self, name, a):
        """Ghost zones of grav_old / grav_new (`name`) of every box, after interpolate_monopole_grav has filled the whole FABs.
        A ghost zone under a sibling's valid zone already holds the sibling's bits (same level, same radial array, same function
        of the index).  Ghost zones covered only by the coarser level: the coarse Gravity_Type data -- grav_old / grav_new of its
        last advance -- interpolated in time ((1 - a) old + a new) and space (cell_cons_interp, Castro_setup.cpp:352-364,
        414-416); the interpolation runs over the whole ghost shell inside the domain and the siblings' valid zones are copied
        over it, as FillPatch does.  Ghost zones outside the domain: the Gravity_Type boundary fill (Castro_setup.cpp:614-622)."""
        h = self.hydro
        if self.plain_base:
            for b in self.mine:
                h.grav_bc_fill(getattr(b, name), b.gravbox, b.geom)
            return
        if self.amr.nranks > 1:
            X = self.amr._xrun
            X([("grav_lincomb", b, p, lo, hi, a) for b in self.boxes for p, (lo, hi) in b.gsrc + b.gsrc_valid], 3)
            for b in (self.mine if self.l > 0 else ()):
                for lo, hi in b.gshell:
                    h.cc_interp(b.gctmp, b.gcbox, getattr(b, name), b.gravbox, lo, hi, 3)
            if self.l > 0:
                X([("grav_copy", b, sb, lo, hi, (name, sh)) for b in self.boxes for sb, (lo, hi), sh in b.gsib], 3)
            for b in self.mine:
                h.grav_bc_fill(getattr(b, name), b.gravbox, b.geom)
            return
        if self.batched and self._level_calls():
            mk, P = h.make_ops, self.params
            if self.l > 0:
                for key, attr in (("grav_lincomb_ghost", "gsrc"), ("grav_lincomb_valid", "gsrc_valid")):
                    ops = self._cached_ops((key,), (), lambda attr=attr: mk(
                        [(L.OP_LINCOMB, 0, 3, lo, hi, 0.0, 0.0, (b.gctmp, b.gcbox), (p.grav_old, p.gravbox), (p.grav_new, p.gravbox))
                         for b in self.boxes for p, (lo, hi) in getattr(b, attr)]))
                    arr, n = ops
                    for i in range(n):
                        arr[i].a, arr[i].b = 1.0 - a, a
                    h.fab_ops(ops, params=P)
                h.fab_ops(self._cached_ops(("grav_shell", name), (), lambda: mk(
                    [(L.OP_INTERP, 0, 3, lo, hi, 0.0, 0.0, (getattr(b, name), b.gravbox), (b.gctmp, b.gcbox), None)
                     for b in self.boxes for lo, hi in b.gshell])), params=P)
                h.fab_ops(self._cached_ops(("grav_sib", name), (), lambda: mk(
                    [(L.OP_COPY, 0, 3, lo, hi, 0.0, 0.0, (getattr(b, name), b.gravbox), (getattr(sb, name), _shift(sb.gravbox, sh)), None)
                     for b in self.boxes for sb, (lo, hi), sh in b.gsib])), params=P)
            for b in self.boxes:
                if b.grav_at_edge:
                    h.grav_bc_fill(getattr(b, name), b.gravbox, b.geom)
            return
        for b in (self.boxes if self.l > 0 else ()):
            for p, (lo, hi) in b.gsrc + b.gsrc_valid:           # ghost zones of the parents first, valid zones last
                h.lincomb(b.gctmp, b.gcbox, 1.0 - a, p.grav_old, p.gravbox, a, p.grav_new, p.gravbox, 3, lo, hi)
            for lo, hi in b.gshell:
                h.cc_interp(b.gctmp, b.gcbox, getattr(b, name), b.gravbox, lo, hi, 3)
        for b in self.boxes:
            for sb, (lo, hi), sh in (b.gsib if self.l > 0 else ()):
                h.copy(getattr(b, name), b.gravbox, getattr(sb, name), _shift(sb.gravbox, sh), lo, hi)
            h.grav_bc_fill(getattr(b, name), b.gravbox, b.geom)

    def create_source_corrector(self):
        """Castro::create_source_corrector on a level of boxes (Castro.cpp:3780-3818): AmrLevel::FillPatch(Source_Type at its old
        time -- after the swap that is the new-time corrector of the LAST advance --, components UMX .. UMZ, NUM_GROW_SRC ghost
        zones): the valid zones of every box from its own data, ghost zones from the other boxes of the level, from the coarser
        level's Source_Type data interpolated in time and space (the FillPatch of fill_source) and from the physical boundaries;
        then x 2 / lastDt.  The factor dt / 2 is applied in src_to_prim (Castro_ctu.cpp:493-497)."""
        g = 3                                   # NUM_GROW_SRC
        for b in self.mine:
            c, n = b.source_corrector, b.n
            c.zero_()
            c[1:4, g:g + n[2], g:g + n[1], g:g + n[0]] = b.new_source[1:4]
        self.fill_source("source_corrector")
        for b in self.mine:
            c = b.source_corrector
            c[0].zero_()                        # the FillPatch of the reference moves the three momentum components only
            c[4:].zero_()
            c.mul_(2.0 / self.lastDt)

    def _advance_with_sources(self, time, dt):
        if self.params.source_term_predictor == 1 and not self._in_retry:
            # not on the attempt that follows a rejected one: the data it is made from are gone by then (Castro_advance_ctu.cpp:60-62)
            self.create_source_corrector()
        return self._advance_with_sources_impl(time, dt)

    def _advance_with_sources_impl(self, time, dt):
        """do_advance_ctu with old- and new-time gravity / rotation sources (Castro_advance_ctu.cpp:94-143, 156-274), stage by
        stage over the boxes of the level.  The source stages are the single-level driver's own: Castro._source_stage box by
        box, or Castro._sources_one_pass over the level's boxes."""
        h = self.hydro
        lvl = self._source_level_calls()        # the per-box stages as one library call per level (castro_amd_sources_mf)
        G = self.amr.gravity

        def sources(stage):
            if G is not None:
                # construct_old_gravity in front of the old-time sources (Castro_advance_ctu.cpp:122), construct_new_gravity in
                # front of the new-time ones (:258): level-wide, every coarser level at this level's time
                if stage == 0:
                    G.get_old_grav_vector(self.l, time, self.alpha)
                else:
                    G.get_new_grav_vector(self.l, time + dt, self.alpha + dt / self._dt_parent if self.l > 0 else 1.0)
            if lvl is None:
                for b in self.mine:
                    b._source_stage(stage, dt)
                return
            sp = tuple(t.data_ptr() for b in self.mine for t in (b.S_old_b, b.S_new_b))
            gf = None
            if G is not None:                   # Gravity_Type FABs keep their storage between regrids
                gf = self._cached_ops(("grav_fabs",), (), lambda: (h.make_grav_fabs([(b.grav_old, b.gravbox) for b in self.mine]),
                                                                   h.make_grav_fabs([(b.grav_new, b.gravbox) for b in self.mine])))
            lvl._sources_one_pass(stage, dt, self._cached_ops((("src_old", "src_new")[stage],), sp, lambda: h.make_source_boxes(
                [b._source_spec(stage) for b in self.mine])), **({} if gf is None else {"grav_fabs": gf}))
        sources(0)
        self.fill_source("old_source")
        predictor = self.params.source_term_predictor == 1
        def hydro(b):
            # b.hydro is the context this box's call runs on (one of the stream pool's, _hydro_calls)
            if predictor:
                b.hydro.set_source_corrector(b.source_corrector, b.sbox)
            try:
                b.construct_ctu_hydro_source(time, dt, src=b.old_source)
            finally:
                if predictor:
                    b.hydro.set_source_corrector(None, None)      # the context must not keep a pointer into this box's tensor
            b._flux_clear = False
        if predictor or not self._hydro_level(time, dt, with_src=True):
            self._hydro_calls(hydro)
        self._clean_reduce_new()
        self.amr.comm.allreduce_min(self.red)
        bad = density_failure(self._read_red()[1], self.params)
        if bad:
            return bad
        sources(1)
        new_dt = self.estTimeStep()
        if self.params.change_max * new_dt < dt:
            return False, "timestep validity check failed", None
        return True, "", new_dt

    def _source_level_calls(self):
        """The box whose gravity / rotation settings stand for the level when the source stages go out as one library call per
        level (device backend, every box on this rank, the same settings in every box -- they come from one set of inputs);
        None: box by box."""
        if not (self._level_calls() and self.mine and hasattr(self.hydro, "sources_mf")):
            return None
        if os.environ.get("CASTRO_AMD_SOURCES_ONE_PASS", "1") == "0" and (self.amr.gravity is not None or self.mine[0].sponge is not None):
            return None                         # the separate-call form of the gravity / sponge sources (A/B and tests)
        b0 = self.mine[0]
        if b0.monopole and not hasattr(self.hydro, "sources_mf_g"):
            return None
        for b in self.mine:
            if (b.do_grav != b0.do_grav or b.monopole != b0.monopole or (b.do_grav and (tuple(b.grav) != tuple(b0.grav) or b.grav_source_type != b0.grav_source_type))
                    or b.rotation is not b0.rotation or b.sponge is not b0.sponge):
                return None
        return b0

    def _state_boxes(self, which):
        sp = tuple(getattr(b, which).data_ptr() for b in self.mine)
        return self._cached_ops(("state_boxes", which), sp, lambda: self.hydro.make_state_boxes(
            [(b.lo, b.hi, (getattr(b, which), b.gbox)) for b in self.mine]))

    def _clean_reduce_new(self):
        """clean_state_reduce of S_new of every box into the level's reduction vector."""
        h = self.hydro
        if self._level_calls() and len(self.mine) > 1 and hasattr(h, "clean_state_reduce_mf"):
            h.clean_state_reduce_mf(self._state_boxes("S_new_b"), self.mine[0].geom, self.params, self.red, ntimes=1)
            return
        for b in self.mine:
            h.clean_state_reduce(b.S_new_b, b.gbox, b.lo, b.hi, b.geom, b.params, self.red, ntimes=1)

    # ---- Castro::advance over the boxes of the level (Castro_advance.cpp:19-121) ----------------------
    def _swap_state_time_levels(self):
        for b in self.mine:
            b._swap_state_time_levels()
        G = self.amr.gravity
        if G is not None and hasattr(G, "swap_level"):          # PhiGrav_Type of a PoissonGravity: phi_old <- phi_new
            G.swap_level(self.l)

    def _zero_fluxes(self):
        for b in self.mine:
            b._zero_fluxes()

    def _save_old_state(self):
        return [b.S_old_b.clone() for b in self.mine]

    def _restore_old_state(self, prev):
        if self.amr.update_sources_after_reflux and self.have_sources:
            # keep_prev_state (Castro_advance_ctu.cpp:722-755): the advance ended with more than one subcycle and a reflux may
            # re-evaluate the new-time sources, which belong to the LAST subcycle.  Of the state types only State_Type differs
            # here: old_source and grav_old are rebuilt by every subcycle and are the last one's as they stand.
            self._last_old = [b.S_old_b.clone() for b in self.mine]
        for b, p in zip(self.mine, prev):
            b.S_old_b.copy_(p)

    # ---- Castro::reflux with castro.update_sources_after_reflux (Castro.cpp:2773-2868) ----------------------------------
    def renew_sources(self):
        """The new-time sources of this level again, after a reflux has changed S_new and the mass fluxes: S_new += -dt x
        new_source, clean_state, do_new_sources(apply = true) -- with dt and the old data of the level's last advance, of its
        last subcycle if a retry split it.  The gravity field is the one that advance constructed (construct_new_gravity belongs
        to do_advance_ctu).  One call of stage 1 | SOURCES_AFTER_REFLUX for the level where the source stages go out level-wide, else box by box."""
        if not self.have_sources or not self.mine:
            return
        h, dt = self.hydro, self.lastDt
        keep = None
        if getattr(self, "_last_old", None) is not None:
            keep = [b.S_old_b.clone() for b in self.mine]
            for b, p in zip(self.mine, self._last_old):
                b.S_old_b.copy_(p)
        lvl = self._source_level_calls()
        if lvl is not None:
            sp = tuple(t.data_ptr() for b in self.mine for t in (b.S_old_b, b.S_new_b))
            gf = None
            if self.amr.gravity is not None:
                gf = self._cached_ops(("grav_fabs",), (), lambda: (h.make_grav_fabs([(b.grav_old, b.gravbox) for b in self.mine]),
                                                                   h.make_grav_fabs([(b.grav_new, b.gravbox) for b in self.mine])))
            lvl._sources_one_pass(1 | L.SOURCES_AFTER_REFLUX, dt, self._cached_ops(("src_new",), sp, lambda: h.make_source_boxes(
                [b._source_spec(1) for b in self.mine])), **({} if gf is None else {"grav_fabs": gf}))
        else:
            for b in self.mine:
                if hasattr(h, "apply_source"):
                    h.apply_source(b.S_new_b, b.gbox, b.S_new_b, b.gbox, -dt, b.new_source, b.bx, NSRC, b.lo, b.hi, b.params, ntimes=1)
                else:
                    h.saxpy(b.S_new_b, b.gbox, -dt, b.new_source, b.bx, NSRC, b.lo, b.hi)
                    h.clean_state(b.S_new_b, b.gbox, b.lo, b.hi, b.params, ntimes=1)
                b._source_stage(1, dt)
        if keep is not None:
            for b, p in zip(self.mine, keep):
                b.S_old_b.copy_(p)
        self.invalidate_estimate()              # S_new has been written outside the level's advance

    def advance(self, time, dt):
        self._last_old = None                   # the old data of the last retry subcycle of this advance (_restore_old_state)
        return Castro.advance(self, time, dt)

    subcycle_advance_ctu = Castro.subcycle_advance_ctu

    def _pointmass_update(self):
        """Castro::pointmass_update at the end of this level's advance (Castro_advance.cpp:102-107): it acts on the finest EXISTING
        level only (level == parent->finestLevel()) -- on every one of its subcycles, and on level 0 while nothing finer exists.
        S_old_b of every box is the old state of the whole advance.  Collective over the ranks.  True if it ran."""
        pm = self.amr.pm
        if pm is None or not pm.fix_solution or self.l != len(self.amr.lev) - 1:
            return False
        h = self.hydro
        specs = [(b.lo, b.hi, (b.S_old_b, b.gbox), (b.S_new_b, b.gbox)) for b in self.mine]
        pm.update(h, self.amr.comm, h.make_pointmass_boxes(specs), self.amr.gravity.problem_center(), self.geom)
        self.invalidate_estimate()              # S_new has been written outside the update pass
        return True

    # ---- tracer particles (castro_amd/particles.py) -----------------------------------------------------------------------
    def _tracer_boxes(self, which):
        """the make_tracer_boxes table of S_half_b / S_new_b of the boxes of the level, in box order (a particle's `grid`)"""
        key = (which,) + tuple(getattr(b, which).data_ptr() if b.owned else 0 for b in self.boxes)     # no FAB on another rank's box
        tabs = self.__dict__.setdefault("_tracer_tabs", {})
        if key not in tabs:
            if len(tabs) > 8:
                tabs.clear()
            tabs[key] = self.hydro.make_tracer_boxes([(b.lo, b.hi, (getattr(b, which), b.gbox) if b.owned else None)
                                                      for b in self.boxes])
        return tabs[key]

    def _advance_particles(self, time, dt):
        """Castro::advance_particles of this level (CastroParticles.cpp:252-281), at the end of its advance: the FillPatch of the
        state at time + dt / 2 into S_half_b of every box -- the valid zones 0.5 old + 0.5 new, the ghost zones through the
        level's fill with the coarse data interpolated in time first (a quarter of the parent's step past this level's old
        time), then in space -- and AdvectWithUcc.  time, dt: those of the whole advance."""
        tr = self.amr.tracers
        if tr is None:
            return
        h = self.hydro
        for b in self.mine:
            h.lincomb(b.S_half_b, b.gbox, 0.5, b.S_old_b, b.gbox, 0.5, b.S_new_b, b.gbox, NUM_STATE, b.lo, b.hi)
        keep = self.alpha
        if self.l > 0:
            self.alpha = self._alpha0 + 0.25
        self.fill("S_half_b")
        self.alpha = keep
        tr.advect(self.l, self._tracer_boxes("S_half_b"), self.geom, dt, ng=self._iteration)

    def _hydro_calls(self, fn):
        """fn(b) -- the hydro update of one box -- for every box of this rank.  The boxes of a level are independent
        there, and one small box fills a fraction of the chip (a 32^3 box is 64 workgroups of 256 CUs' worth), so with
        the device backend up to `box_streams` boxes are in flight at once, each on its own stream with its own scratch
        context; the level's reductions are atomic minima into one pair, the streams are joined before anything else runs."""
        pool = self.amr._stream_pool(self.l) if len(self.mine) > 1 else None
        if not pool:
            for b in self.mine:
                fn(b)
            return
        main = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(main)
        used = pool[:min(len(pool), len(self.mine))]
        for _, st in used:
            st.wait_event(ev)
        for i, b in enumerate(self.mine):
            ctx, st = pool[i % len(pool)]
            keep, b.hydro = b.hydro, ctx
            try:
                with torch.cuda.stream(st):
                    fn(b)
            finally:
                b.hydro = keep
        for _, st in used:
            main.wait_stream(st)

    def do_advance_ctu(self, time, dt):
        """Castro::do_advance_ctu (Castro_advance_ctu.cpp:15-397) with every stage done for all boxes before the next."""
        if self.l > 0 and time != self._t0:
            # a later subcycle of a retried step: the coarse data are interpolated to ITS old time, not the step's
            self.alpha = self._alpha0 + (time - self._t0) / self._dt_parent
        if self._pending_cleans > 0:           # see Castro.do_advance_ctu
            self._clean_boxes("S_old_b", self._pending_cleans)
        self._pending_cleans = 0
        self._cached_est = None
        self.red.fill_(1.e200)
        self.fill("S_old_b")
        if self.have_sources:
            return self._advance_with_sources(time, dt)
        if not self._hydro_level(time, dt):
            def hydro(b):
                b.construct_ctu_hydro_source(time, dt, fuse_clean=self.fuse_clean)
                b._flux_clear = False
            self._hydro_calls(hydro)
        if not self.fuse_clean:
            self._clean_reduce_new()
        self.amr.comm.allreduce_min(self.red)                 # the level's minima over the ranks that hold its boxes
        est_last, rho_min, est = self._read_red()    # [2]: the estimate after the first clean_state (the only one here
                                                      # unless post_timestep's rode along: then [0] is the one after it)
        if self._post_clean_done:
            # the state leaves this advance as post_timestep will leave it (finest level, whole-step attempt): its CFL
            # estimate is what estTimeStep would reduce again from the same zones (Castro.step: _next_est)
            self._cached_est = est_last
        bad = density_failure(rho_min, self.params)
        if bad:
            return bad
        new_dt = self.fixed_dt if self.fixed_dt > 0.0 else min(self.max_dt, est * self.params.cfl)
        if self.params.change_max * new_dt < dt:
            return False, "timestep validity check failed", None
        return True, "", new_dt

    def invalidate_estimate(self):
        """S_new of this level has been written outside its own advance (avgDown from a finer level, reflux, initData, a
        regrid that filled it, a user's edit of b.S_new()): the CFL estimate cached from the fused post-update pass no longer
        describes it and estTimeStep reduces over the zones again, as the reference always does (Castro.cpp:1507-1626)."""
        self._cached_est = None

    def estTimeStep(self):
        if getattr(self, "_cached_est", None) is not None and self._post_clean_done and self.boxes:
            return min(self.max_dt, checked_estimate(self._cached_est) * self.params.cfl)
        self.red.fill_(1.e200)
        if self._level_calls() and len(self.mine) > 1 and hasattr(self.hydro, "estdt_cfl_mf"):
            self.hydro.estdt_cfl_mf(self._state_boxes("S_new_b"), self.mine[0].geom, self.params, self.red)
        else:
            for b in self.mine:
                self.hydro.estdt_cfl(b.S_new_b, b.gbox, b.lo, b.hi, b.geom, b.params, self.red)
        self.amr.comm.allreduce_min(self.red)
        return min(self.max_dt, checked_estimate(self._read_red()[0], empty_ok=not self.boxes) * self.params.cfl)

    def clean_new(self):
        self._clean_boxes("S_new_b", 1)

    def _level_calls(self):
        """One library call per level instead of one per box (castro_amd_ctu_hydro_mf, castro_amd_fab_ops_p): the device
        backend with every box on this rank; CASTRO_AMD_LEVEL_CALLS=0 keeps the per-box calls."""
        return (getattr(self, "batched", False) and hasattr(self.hydro, "construct_ctu_hydro_source_mf")
                and os.environ.get("CASTRO_AMD_LEVEL_CALLS", "1") != "0")

    def _clean_boxes(self, which, ntimes):
        """Castro::clean_state x ntimes on the valid zones of S_old_b / S_new_b (`which`) of every box of this rank."""
        if not self._level_calls() or len(self.mine) < 2:
            for b in self.mine:
                b.clean_state(getattr(b, which), ntimes)
            return
        sp = tuple(getattr(b, which).data_ptr() for b in self.mine)
        ops = self._cached_ops(("clean", which, ntimes), sp, lambda: self.hydro.make_ops(
            [(L.OP_CLEAN, 0, NUM_STATE, b.lo, b.hi, float(ntimes), 0.0, (getattr(b, which), b.gbox), (getattr(b, which), b.gbox), None)
             for b in self.mine]))
        self.hydro.fab_ops(ops, params=self.params)

    def _hydro_level(self, time, dt, with_src=False):
        """The hydro update of every box of the level through ONE library call (the MFIter loop of
        construct_ctu_hydro_source in C++: boxes dealt round robin to the contexts / streams of the box-stream pool, forked
        from and joined to the current stream inside the call).  False: not applicable, the caller loops over the boxes.
        with_src (_advance_with_sources_impl, between the two source stages): every box hands its old-time source FAB to the
        call, which traces it and adds the hydro update to the S_new that stage 0 has prepared; the new-time stage follows, so
        nothing is fused behind it."""
        if not self._level_calls() or not self.mine:
            return False
        fa = [bool(b.flux_assign and b._flux_clear) for b in self.mine]
        if any(x != fa[0] for x in fa) or any(b.fuse_post_clean for b in self.mine) or any(b.have_sources != with_src for b in self.mine):
            return False
        sp = tuple(t.data_ptr() for b in self.mine for t in (b.S_old_b, b.S_new_b))
        if with_src:
            boxes = self._cached_ops(("hydro_mf_src",), sp, lambda: self.hydro.make_hydro_boxes(
                [(b.bx, b.bx, (b.S_old_b, b.gbox), (b.S_new_b, b.gbox), b.fluxes, b.flux_boxes, b.mass_fluxes, (b.old_source, b.sbox))
                 for b in self.mine]))
            pool = self.amr._stream_pool(self.l) if len(self.mine) > 1 else None
            self.hydro.construct_ctu_hydro_source_mf(pool, boxes, self.mine[0].geom, self.params, time, dt, update_from_sborder=False,
                                                     flux_assign=fa[0], clean_ntimes=0, red=None)
            for b in self.mine:
                b._flux_clear = False
            return True
        boxes = self._cached_ops(("hydro_mf",), sp, lambda: self.hydro.make_hydro_boxes(
            [(b.bx, b.bx, (b.S_old_b, b.gbox), (b.S_new_b, b.gbox), b.fluxes, b.flux_boxes, b.mass_fluxes) for b in self.mine]))
        pool = self.amr._stream_pool(self.l) if len(self.mine) > 1 else None
        # On the finest level nothing touches S_new between the update and post_timestep's clean_state (no reflux, no
        # avgDown into it; FluxRegFineAdd only reads the fluxes): an attempt at the whole step takes that clean_state into the
        # fused pass, like the single-level driver (Castro.construct_ctu_hydro_source), instead of a sweep of its own
        post = bool(self.fuse_clean and getattr(self, "fuse_post_level", False) and getattr(self, "_whole_step", False))
        if post:
            self._post_clean_done = True
        self.hydro.construct_ctu_hydro_source_mf(pool, boxes, self.mine[0].geom, self.params, time, dt, update_from_sborder=True,
                                                 flux_assign=fa[0], clean_ntimes=(2 if post else 1) if self.fuse_clean else 0,
                                                 red=self.red if self.fuse_clean else None)
        for b in self.mine:
            b._flux_clear = False
        return True


_TAG_KINDS = {"value_greater": 0, "value_less": 1, "gradient": 2, "relative_gradient": 3}
_FIELDS = {"density": 0, "xmom": 1, "ymom": 2, "zmom": 3, "rho_E": 4, "rho_e": 5, "Temp": 6, "rho_X": 7}


class CastroAmr(CheckpointMixin):
    def __init__(self, n_cell, patch_crse=None, prob_lo=(0., 0., 0.), prob_hi=(1., 1., 1.), lo_bc=(2, 2, 2), hi_bc=(2, 2, 2),
                 params=None, make_hydro=None, make_params=None, refine=None, regrid_int=2, n_error_buf=1,
                 blocking_factor=8, patches=None, max_level=1, cluster=False, grid_eff=0.7, max_grid_size=128,
                 do_grav=False, const_grav=0.0, grav_source_type=4, rotation=None, comm=None, base_grid=None, box_streams=4,
                 diffusion=None, sum_interval=-1, show_center_of_mass=False, diag_dir=None, gravity_type="constant", gravity=None,
                 sponge=None, use_point_mass=False, point_mass=0.0, point_mass_fix_solution=False, ext_bc=None,
                 update_sources_after_reflux=False, tracers=None, check_int=-1, check_file="chk", poisson=None):
        """poisson: refused -- the keyword of the single-level driver (castro_amd.Castro); a hierarchy takes gravity=PoissonGravity(...).
        check_int, check_file (amr.check_int, default -1: never / amr.check_file): evolve() writes the checkpoint
        check_file + "%05d" % nstep after every coarse step with nstep % check_int == 0, in the background
        (castro_amd/checkpoint.py: writeCheckpoint, restart -- the box lists of every level come from the file, nothing is
        clustered again --, checkpoint_wait, close).
        tracers: a castro_amd.TracerParticles (castro.do_tracer_particles = 1) spanning the levels: advected at the end of
        every level's advance, redistributed and timestamped at the end of its post_timestep and after every regrid, as in
        castro_amd.Castro; with the boxes dealt over ranks every rank holds the particles of its boxes (castro_amd/particles.py).
        update_sources_after_reflux: castro.update_sources_after_reflux.  True is the reference's default (1) and the setting
        that follows it: after the reflux of post_timestep the flux registers are added to the coarse level's fluxes (mass
        fluxes = their density component) and both levels take their new-time sources out of S_new, clean it, and evaluate and
        apply them again from the refluxed state and the corrected mass fluxes (Castro.cpp:2612-2644, 2762-2868).  False (the
        default here): the reflux ends with the flux correction of the state.
        ext_bc: _lib.make_ext_bc(...) -- the boundary overrides of the state fill (hydrostatic Inflow faces, the ambient state
        beyond Outflow faces) on every box of every level that reaches the boundary, as in castro_amd.Castro; the hydrostatic
        fill assumes constant gravity (not with gravity=MonopoleGravity(...)).
        use_point_mass, point_mass, point_mass_fix_solution: as in castro_amd.Castro, with gravity=MonopoleGravity(...) -- ONE
        point mass per hierarchy (self.point_mass reads the device value), its field added after the Gravity_Type FillPatch of
        every level, Castro::pointmass_update after every advance of the finest existing level.  Constant gravity plus a point
        mass is not built for AMR levels (the Gravity_Type FillPatch tables exist for monopole gravity only).
        sponge: _lib.make_sponge(timescale, ...) -- castro.do_sponge = 1 on every box of every level (zone-local: a refined
        level needs nothing from the coarser one), as in castro_amd.Castro.
        gravity: castro_amd.MonopoleGravity(drdxfac=..., Gconst=...) with do_grav=True -- monopole self-gravity on every
        level (castro_amd/gravity.py: the object spans the levels like the reference's Gravity); or
        castro_amd.PoissonGravity(..., max_solve_level=None) -- Poisson self-gravity with every level solving for itself
        (gravity.no_sync = 1, gravity.no_composite = 1): one rank, level 0 ONE box, a refined level one box or several (fixed
        patches=[[box, ...]] or refine= with cluster=True; a level of several is solved as one array over their bounding box),
        every refined box inside the domain; phi_grav(level) -- phi_grav_level(level) for a level of several boxes -- and
        poisson_stats(level) read the potentials and the cycle counts, close() gives the multigrid plans back.
        gravity_type: "constant" only (the bare string "monopole" carries neither drdxfac nor Gconst and is refused).
        sum_interval, show_center_of_mass, diag_dir: as in castro_amd.Castro -- sum_integrated_quantities() over the composite
        grid after initData and after every coarse step with nstep % sum_interval == 0 (self.diag_history, the three data logs).
        base_grid = (gx, gy, gz): level 0 as gx x gy x gz equal boxes instead of one (amr.max_grid_size on the base level);
        with `comm` they are dealt over the ranks like the boxes of the refined levels.
        comm: a castro_amd.DistComm to spread the boxes of every refined level over its ranks (box i of level l on rank
        (i + l) mod size, level 0 on rank 0 unless base_grid cuts it up): every rank builds the same hierarchy, holds the
        memory of its own boxes only and moves box-to-box data (coarse data under fine ghost shells, sibling ghost zones,
        coarse fluxes for the registers, registers for the reflux, averaged-down zones) with one grouped RCCL
        point-to-point exchange per pass.
        patch_crse = (lo, hi): the coarse zones covered by a FIXED refined box;
        patches = [entry, ...]: one entry per refined level, a box (lo, hi) or a list of boxes in the zones of the
        level below it (amr.max_level = len(patches)); or
        refine = [(field, kind, value), ...] like amr.refinement_indicators (field: a state name or a pointwise
        derived field such as pressure, kind:
        value_greater | value_less | gradient | relative_gradient) for boxes that follow the tags up to
        amr.max_level = max_level: one bounding box per level, or with cluster=True the Berger-Rigoutsos boxes
        (amr.grid_eff, amr.blocking_factor and amr.max_grid_size in zones of the new level)."""
        if poisson is not None:
            raise NotImplementedError("CastroAmr: Poisson gravity (poisson=...) is built for a single level only -- the level "
                                      "solves, gravity_sync and the composite correction of the hierarchy are a follow-up; use "
                                      "castro_amd.Castro")
        from .gravity import PoissonGravity, refuse_for_poisson
        if diffusion is not None and isinstance(gravity, PoissonGravity):
            raise ValueError("CastroAmr: gravity=PoissonGravity(...) not together with diffusion=...: thermal diffusion is built for "
                             "a single level only")
        if diffusion is not None:
            # the operator of a refined level needs AMReX's coarse-fine boundary stencil [3P], which is not restated
            raise NotImplementedError("CastroAmr: thermal diffusion (diffusion=...) is built for a single level only; "
                                      "use castro_amd.Castro")
        if gravity_type not in ("constant", "monopole"):
            raise ValueError("gravity_type must be \"constant\" or \"monopole\", not %r" % (gravity_type,))
        if gravity_type == "monopole":
            raise NotImplementedError("CastroAmr: gravity_type=\"monopole\" is the single-level form (castro_amd.Castro); the level "
                                      "combination and the time interpolation of Gravity::make_radial_gravity "
                                      "(Gravity.cpp:2962-3127) are reached with gravity=castro_amd.MonopoleGravity(drdxfac=..., "
                                      "Gconst=...)")
        if gravity is not None:
            from .gravity import MonopoleGravity
            if not isinstance(gravity, (MonopoleGravity, PoissonGravity)):
                raise TypeError("gravity must be a castro_amd.MonopoleGravity or a castro_amd.PoissonGravity, not %r" % (type(gravity),))
            if not do_grav:
                raise ValueError("gravity=%s(...) needs do_grav=True" % type(gravity).__name__)
            if isinstance(gravity, PoissonGravity):
                refuse_for_poisson("CastroAmr: ", comm, base_grid, use_point_mass, check_int, ext_bc,
                                   L.make_geom(n_cell, prob_lo, prob_hi, lo_bc, hi_bc))
            gravity.bind(self, lo_bc, hi_bc)
        self.gravity = gravity
        self.pm = None
        self.update_sources_after_reflux = bool(update_sources_after_reflux)
        if use_point_mass:
            if not do_grav:
                raise ValueError("use_point_mass needs do_grav=True: the point mass is a term of the gravity vector")
            if gravity is None:
                raise NotImplementedError("CastroAmr: a point mass with constant gravity is not built for AMR levels (their "
                                          "Gravity_Type FillPatch exists for gravity=MonopoleGravity(...) only); use "
                                          "castro_amd.Castro, or monopole gravity")
        if patch_crse is not None:
            assert patches is None
            patches = [patch_crse]
        assert (patches is None) != (refine is None), "give either fixed patches or refinement indicators"
        from .castro import SingleComm
        self.comm = comm if comm is not None else SingleComm()
        self.rank, self.nranks = self.comm.rank, self.comm.size
        self.tracers = tracers
        self._mk = (lambda: None) if make_hydro is None else make_hydro
        self.params = params if params is not None else (make_params() if make_params else L.default_params())
        self._kw = dict(prob_lo=prob_lo, prob_hi=prob_hi, lo_bc=lo_bc, hi_bc=hi_bc, params=self.params, overlap=False,
                        do_grav=do_grav, const_grav=const_grav, grav_source_type=grav_source_type, rotation=rotation)
        if gravity is not None:
            self._kw["gravity"] = gravity
        if sponge is not None:
            self._kw["sponge"] = sponge
        if ext_bc is not None:
            self._kw["ext_bc"] = ext_bc
        self.n_cell = tuple(n_cell)
        self.periodic = tuple(lo_bc[d] == 0 and hi_bc[d] == 0 for d in range(3))
        # boxes of a level whose hydro updates may be in flight at once (device backend); CASTRO_AMD_BOX_STREAMS overrides
        self.box_streams = int(os.environ.get("CASTRO_AMD_BOX_STREAMS", box_streams))
        self._hydros = []
        if tracers is not None:
            from .particles import need_migration
            need_migration(self._hydro_for(0), self.comm)   # NotImplementedError on more than one rank without the migration
        if base_grid is None or tuple(base_grid) == (1, 1, 1):
            base = Castro(n_cell, hydro=self._hydro_for(0), alloc=(self.rank == 0), **self._kw)
            base.owner = 0
            if base.have_sources and base.owned:
                base.new_source_g = base.hydro.alloc(NSRC, *base.sbox)
            self.lev = [_Level(self, 0, [base])]                      # lev[0] covers the domain
            self.lev[0].bind()
            if gravity is not None:
                gravity.check_level(0, base.geom)
        else:
            gx = tuple(int(x) for x in base_grid)
            assert all(self.n_cell[d] % gx[d] == 0 and self.n_cell[d] // gx[d] >= 2 * NUM_GROW for d in range(3)), \
                "base_grid must divide the domain into boxes of at least %d zones a side" % (2 * NUM_GROW)
            nb = tuple(self.n_cell[d] // gx[d] for d in range(3))
            self.lev = []
            boxes = []
            for i, (kz, jy, ix) in enumerate(itertools.product(range(gx[2]), range(gx[1]), range(gx[0]))):
                lo = (ix * nb[0], jy * nb[1], kz * nb[2])
                hi = tuple(lo[d] + nb[d] - 1 for d in range(3))
                owner = i % self.nranks
                b = _Patch(self.n_cell, hydro=self._hydro_for(0), box=(lo, hi), alloc=(owner == self.rank), **self._kw)
                b.owner = owner
                boxes.append(b)
            lev0 = _Level(self, 0, boxes)
            for b in boxes:
                b.bind(lev0, None)
            self.lev.append(lev0)
            lev0.bind()
            if gravity is not None:
                gravity.check_level(0, lev0.geom)
        if tracers is not None:
            tracers.bind(self._hydro_for(0), self.lev[0].geom, self.comm)
        if use_point_mass:
            from .gravity import PointMass
            self.pm = gravity.point_mass = PointMass(self._hydro_for(0), point_mass, point_mass_fix_solution, gravity.Gconst)
        self.refine = refine
        self.regrid_int, self.n_error_buf, self.blocking_factor = int(regrid_int), int(n_error_buf), int(blocking_factor)
        self.cluster = bool(cluster)
        self.grid_eff = float(grid_eff) if cluster else 0.0           # 0: the bounding box of the tags is accepted as it is
        self.max_grid_size = int(max_grid_size) if cluster else None
        self.nregrid = 0
        self.max_level = int(max_level) if refine is not None else len(patches or [])
        for pb in (patches or []):
            self._push_level([tuple(map(tuple, pb))] if _is_box(pb) else [tuple(map(tuple, b)) for b in pb])
        self.time, self.nstep = 0.0, 0
        self.dt_level = [0.0] * 16
        self.level_count = [0] * 16                                   # Amr::level_count: steps of a level since its last regrid
        self.check_int, self.check_file = int(check_int), str(check_file)
        from .diag import DiagLog
        self.diag = DiagLog(sum_interval, show_center_of_mass, diag_dir, io_rank=self.rank == 0)
        self._diag_out = None

    # ---- gravity=PoissonGravity(...): the level solves (castro_amd/gravity.py) ------------------------------------------------
    def _poisson_gravity(self, what):
        from .gravity import PoissonGravity
        if not isinstance(self.gravity, PoissonGravity):
            raise RuntimeError("%s needs CastroAmr(do_grav=True, gravity=PoissonGravity(...))" % what)
        return self.gravity

    def phi_grav(self, level=0, new=True):
        """PhiGrav_Type of `level`: the potential of its last new-time (or old-time) construction as a (1, nz + 2, ny + 2, nx + 2)
        tensor.  A level that solves keeps the boundary values ON the faces of its box in the ghost zone (edges and corners: 0
        on a refined level); a level above max_solve_level holds the interpolated coarse potential in every zone."""
        return self._poisson_gravity("phi_grav()").phi_level(level, new)

    def phi_grav_level(self, level=0, new=True):
        """PhiGrav_Type of a level of any number of boxes: (box, phi, covered) as numpy -- the bounding box (lo, hi) of the level's
        boxes, the level's potential on its zones (nz, ny, nx), and which of them lie in a box of the level.  A level of several
        boxes keeps its potential as this one array; the zones that are not covered are never written by its solve."""
        return self._poisson_gravity("phi_grav_level()").phi_level_boxes(level, new)

    def poisson_stats(self, level=0):
        """{"first", "old", "new"} of `level`: V-cycles, final residual norm and norm history of the first solve of the level
        and of its last old- and new-time solves (None where none was made)"""
        return self._poisson_gravity("poisson_stats()").stats_level(level)

    use_point_mass = property(lambda self: self.pm is not None)
    point_mass = property(lambda self: self.pm.value() if self.pm is not None else None,
                          doc="castro::point_mass as the device holds it (None without use_point_mass)")
    # views used by the tests and the plotfile writer
    crse = property(lambda self: self.lev[0])
    fine = property(lambda self: self.lev[1] if len(self.lev) > 1 else None)
    levels = property(lambda self: list(self.lev))
    boxes = property(lambda self: [None] + [[b.pbox for b in lev.boxes] for lev in self.lev[1:]])
    # pbox[l]: the box of level l in level l-1 zones when the level has one box, else the list of its boxes
    pbox = property(lambda self: [None] + [bl[0] if len(bl) == 1 else bl for bl in self.boxes[1:]])
    plo = property(lambda self: self.pbox[1][0] if len(self.lev) > 1 else None)
    phi = property(lambda self: self.pbox[1][1] if len(self.lev) > 1 else None)

    def _stream_pool(self, l):
        """[(scratch context, stream)] for the concurrent hydro calls of the boxes of level l, or None (one stream)"""
        if self.box_streams <= 1 or not torch.cuda.is_available() or not hasattr(self._hydro_for(l), "device") \
                or not hasattr(self._hydro_for(l), "lib"):
            return None
        pools = self.__dict__.setdefault("_pools", {})
        if l not in pools:
            from .hydro import HipHydro
            dev = self._hydro_for(l).device
            # the other contexts of a level run the same build of the kernel library as its first one
            pools[l] = [(self._hydro_for(l) if k == 0 else HipHydro(dev.index, numerics=getattr(self._hydro_for(l), "numerics", None)),
                         torch.cuda.Stream(device=dev)) for k in range(self.box_streams)]
        return pools[l]

    def all_hydros(self):
        """Every scratch context this hierarchy launches kernels through: the per-level ones and those of the box-stream
        pools (their latched device status and their kernel profilers are otherwise invisible to the caller)."""
        seen, out = set(), []
        for h in list(self._hydros) + [h for pool in self.__dict__.get("_pools", {}).values() for h, _ in pool]:
            if id(h) not in seen:
                seen.add(id(h))
                out.append(h)
        return out

    def status(self):
        """OR of the latched device status words (rho <= 0 met in ctoprim) of all contexts; clears them."""
        st = 0
        for h in self.all_hydros():
            if hasattr(h, "status"):
                st |= int(h.status())
        return st

    def _hydro_for(self, l):
        while len(self._hydros) <= l:
            h = self._mk()
            if h is None:
                from .hydro import HipHydro
                h = HipHydro(torch.cuda.current_device())
            self._hydros.append(h)
        return self._hydros[l]

    def _make_level(self, l, pboxes):
        """Level l >= 1 covering the boxes `pboxes` (zones of level l-1), with its flux registers."""
        boxes = []
        for i, (plo, phi) in enumerate(pboxes):
            flo = tuple(2 * x for x in plo)
            fhi = tuple(2 * x + 1 for x in phi)
            owner = (i + l) % self.nranks             # level 0 is box 0 of rank 0; one-box levels go round the ranks
            b = _Patch(tuple((2 ** l) * x for x in self.n_cell), hydro=self._hydro_for(l), box=(flo, fhi),
                       alloc=(owner == self.rank), **self._kw)
            b.owner = owner
            boxes.append(b)
        lev = _Level(self, l, boxes)
        for b, pb in zip(boxes, pboxes):
            b.bind(lev, pb)
        return lev

    # ---- box-to-box operations with the boxes spread over ranks ----------------------------------------------
    def _xrun(self, ops, ncomp=NUM_STATE):
        """ops = [(kind, D, S, lo, hi, extra)]: region [lo, hi] of box D from box S.  Both here: the operation itself.
        S here and D elsewhere: the source's contribution is staged in a buffer of the region's shape and sent; D here
        and S elsewhere: it is received and applied, in list order together with the local ones (later entries overwrite
        earlier ones exactly like on one rank).  Every rank walks the same list, so the messages pair up by position."""
        me = self.rank
        sends, recvs, bufs = [], [], {}
        for n, (kind, D, S, lo, hi, extra) in enumerate(ops):
            if D.owner == S.owner:
                continue
            if S.owner == me:
                t = self._xstage(kind, D, S, lo, hi, extra)
                sends.append((D.owner, n, t))
            elif D.owner == me:
                h = D.hydro
                t = h.alloc(ncomp, lo, hi)
                bufs[n] = t
                recvs.append((S.owner, n, t))
        self.comm.exchange(sends, recvs)
        for n, (kind, D, S, lo, hi, extra) in enumerate(ops):
            if D.owner != me:
                continue
            self._xapply(kind, D, S, lo, hi, extra, bufs.get(n))

    def _xstage(self, kind, D, S, lo, hi, extra):
        h = S.hydro
        t = h.alloc(NSRC if kind.startswith("src_") else (3 if kind.startswith("grav_") else NUM_STATE), lo, hi)
        box = (tuple(lo), tuple(hi))
        if kind == "grav_lincomb":             # Gravity_Type data of a parent, interpolated in time
            h.lincomb(t, box, 1.0 - extra, S.grav_old, S.gravbox, extra, S.grav_new, S.gravbox, 3, lo, hi)
            return t
        if kind == "grav_copy":
            name, sh = extra
            h.copy(t, box, getattr(S, name), _shift(S.gravbox, sh), lo, hi)
            return t
        if kind == "src_lincomb":              # Source_Type data of a parent, interpolated in time
            h.lincomb(t, box, 1.0 - extra, S.old_source, S.sbox, extra, S.new_source_g, S.sbox, NSRC, lo, hi)
            return t
        if kind == "src_copy":
            name, sh = extra
            h.copy(t, box, getattr(S, name), _shift(S.sbox, sh), lo, hi)
            return t
        if kind == "lincomb":
            h.lincomb(t, box, 1.0 - extra, S.S_old_b, S.gbox, extra, S.S_new_b, S.gbox, NUM_STATE, lo, hi)
        elif kind == "crse_new":
            h.lincomb(t, box, 0.0, S.S_new_b, S.gbox, 1.0, S.S_new_b, S.gbox, NUM_STATE, lo, hi)
        elif kind == "copy":
            which, sh = extra
            h.copy(t, box, getattr(S, which), _shift(S.gbox, sh), lo, hi)
        elif kind == "crse_init":
            d, side = extra
            h.copy(t, box, S.fluxes[d], S.flux_boxes[d], lo, hi)
        elif kind == "reflux":
            d, side, vol, csh = extra
            reg, rbox = S.regs[(d, side)]
            h.copy(t, box, reg, rbox, lo, hi)
        elif kind == "reg_to_flux":
            d, side, csh = extra
            reg, rbox = S.regs[(d, side)]
            h.copy(t, box, reg, rbox, lo, hi)
        elif kind == "avgdown":
            h.avgdown(S.S_new_b, S.gbox, t, box, lo, hi, NUM_STATE)
        else:
            raise ValueError(kind)
        return t

    def _xapply(self, kind, D, S, lo, hi, extra, buf):
        """the operation on this rank's box D; `buf` holds the staged source when S lives elsewhere"""
        h = D.hydro
        box = (tuple(lo), tuple(hi))
        if kind == "grav_lincomb":
            if buf is None:
                h.lincomb(D.gctmp, D.gcbox, 1.0 - extra, S.grav_old, S.gravbox, extra, S.grav_new, S.gravbox, 3, lo, hi)
            else:
                h.copy(D.gctmp, D.gcbox, buf, box, lo, hi)
        elif kind == "grav_copy":
            name, sh = extra
            if buf is None:
                h.copy(getattr(D, name), D.gravbox, getattr(S, name), _shift(S.gravbox, sh), lo, hi)
            else:
                h.copy(getattr(D, name), D.gravbox, buf, box, lo, hi)
        elif kind == "src_lincomb":
            if buf is None:
                h.lincomb(D.stmp, D.scbox, 1.0 - extra, S.old_source, S.sbox, extra, S.new_source_g, S.sbox, NSRC, lo, hi)
            else:
                h.copy(D.stmp, D.scbox, buf, box, lo, hi)
        elif kind == "src_copy":
            name, sh = extra
            if buf is None:
                h.copy(getattr(D, name), D.sbox, getattr(S, name), _shift(S.sbox, sh), lo, hi)
            else:
                h.copy(getattr(D, name), D.sbox, buf, box, lo, hi)
        elif kind == "lincomb":
            if buf is None:
                h.lincomb(D.ctmp, D.cbox, 1.0 - extra, S.S_old_b, S.gbox, extra, S.S_new_b, S.gbox, NUM_STATE, lo, hi)
            else:
                h.copy(D.ctmp, D.cbox, buf, box, lo, hi)
        elif kind == "crse_new":                                # FillCoarsePatch of a regrid: the parents' new-time data
            if buf is None:
                h.lincomb(D.ctmp, D.cbox, 0.0, S.S_new_b, S.gbox, 1.0, S.S_new_b, S.gbox, NUM_STATE, lo, hi)
            else:
                h.copy(D.ctmp, D.cbox, buf, box, lo, hi)
        elif kind == "copy":
            which, sh = extra
            if buf is None:
                h.copy(getattr(D, which), D.gbox, getattr(S, which), _shift(S.gbox, sh), lo, hi)
            else:
                h.copy(getattr(D, which), D.gbox, buf, box, lo, hi)
        elif kind == "crse_init":
            d, side = extra
            reg, rbox = D.regs[(d, side)]
            src, sbox = (S.fluxes[d], S.flux_boxes[d]) if buf is None else (buf, box)
            h.fluxreg_crse_init(reg, rbox, src, sbox, lo, hi, NUM_STATE, -1.0)
        elif kind == "reflux":
            d, side, vol, csh = extra
            reg, rbox = S.regs[(d, side)] if buf is None else (buf, box)
            h.reflux(D.S_new_b, _shift(D.gbox, csh), reg, rbox, lo, hi, d, side, NUM_STATE, vol)
        elif kind == "reg_to_flux":
            d, side, csh = extra
            reg, rbox = S.regs[(d, side)] if buf is None else (buf, box)
            fbox = _shift(D.flux_boxes[d], csh)
            h.fluxreg_to_flux(D.fluxes[d], fbox, reg, rbox, D.mass_fluxes[d], fbox, lo, hi, NUM_STATE)
        elif kind == "avgdown":
            if buf is None:
                h.avgdown(S.S_new_b, S.gbox, D.S_new_b, D.gbox, lo, hi, NUM_STATE)
            else:
                h.copy(D.S_new_b, D.gbox, buf, box, lo, hi)
        else:
            raise ValueError(kind)

    def gather_level(self, l):
        """[(box, new-time state as a numpy array)] of level l on rank 0 (None elsewhere): for tests and plotfiles"""
        mine = [(b.bx, b.S_new().cpu().numpy()) for b in self.lev[l].mine]
        allv = self.comm.gather_objects(mine)
        if self.rank != 0:
            return None
        got = {bx: a for part in allv for bx, a in part}
        return [(b.bx, got[b.bx]) for b in self.lev[l].boxes]

    def _push_level(self, pboxes):
        lev = self._make_level(len(self.lev), pboxes)
        if self.gravity is not None:
            self.gravity.check_level(len(self.lev), lev.geom)
            if hasattr(self.gravity, "check_boxes"):            # Poisson gravity: boxes inside the domain, nested in the level below
                self.gravity.check_boxes(len(self.lev), lev.box_list(), self.lev[-1].box_list())
        self.lev.append(lev)
        lev.bind()
        self._diag_masks, self._diag_tables = {}, {}    # the zones of the level below that are covered have changed
        if self.gravity is not None:
            self.gravity.reset(len(self.lev) - 1)

    def _drop_fine(self):
        del self.lev[1:]
        self._diag_masks, self._diag_tables = {}, {}
        if self.gravity is not None:
            self.gravity.reset(1)

    # ---- Castro::errorEst (Castro.cpp:3131-3164) ---------------------------------------------------
    def _fill_ghosts_new(self, upto, lbase=0, alpha=1.0):
        """Ghost zones of the new-time data of levels lbase..upto (each FillPatch reads the level below it).  Level
        lbase sits at `alpha` inside its parent's [old, new] interval, the finer ones are synchronised with it."""
        for l in range(lbase, upto + 1):
            self.lev[l].alpha = alpha if l == lbase else 1.0
            self.lev[l].fill("S_new_b")

    def _tags(self, l):
        """(tags, mask, origin): tagged zones and valid zones of level l as 0/1 tensors (on the level's device) over the
        bounding region of its boxes."""
        lev = self.lev[l]
        bl = lev.box_list()
        olo = tuple(min(b[0][d] for b in bl) for d in range(3))
        ohi = tuple(max(b[1][d] for b in bl) for d in range(3))
        h = lev.hydro
        tags, mask = h.alloc(1, olo, ohi)[0], h.alloc(1, olo, ohi)[0]
        for b in lev.boxes:
            sl = tuple(slice(b.lo[d] - olo[d], b.hi[d] - olo[d] + 1) for d in (2, 1, 0))
            mask[sl] = 1.0
            if not b.owned:                                     # its owner tags it; tag_boxes() combines the ranks' tags
                continue
            t = h.alloc(1, b.lo, b.hi)
            for field, kind, value in self.refine:
                if field in _FIELDS:
                    h.error_tag(b.S_new_b, b.gbox, _FIELDS[field], t, (b.lo, b.hi), b.lo, b.hi, _TAG_KINDS[kind], value)
                else:
                    # a derived field (amr.refine.<name>.field_name = pressure, ...): evaluated with one ghost zone
                    # for the gradient kinds, like the reference's derive on a grown box
                    g1 = (tuple(x - 1 for x in b.lo), tuple(x + 1 for x in b.hi))
                    d = h.alloc(1, *g1)
                    center = [0.5 * (b.geom.problo[dd] + b.geom.probhi[dd]) for dd in range(3)]
                    h.derive(field, b.S_new_b, b.gbox, d, g1, 0, g1[0], g1[1], b.geom, b.params, center)
                    h.error_tag(d, g1, 0, t, (b.lo, b.hi), b.lo, b.hi, _TAG_KINDS[kind], value)
            tags[sl] = (t[0] > 0.5).to(tags.dtype)
        return tags, mask, olo

    def _cell_images(self, l, a):
        """Shifts (in blocking cells of level l) to the periodic images of the domain."""
        ext = [(2 ** l) * self.n_cell[d] // a for d in range(3)]
        return list(itertools.product(*[(-ext[d], 0, ext[d]) if self.periodic[d] else (0,) for d in range(3)]))

    def _erode_cells(self, p, o, l, a):
        """p (bool, [z, y, x], origin o in cells of a zones of level l) with every cell removed that has a neighbour
        outside p.  Beyond a physical boundary everything counts as inside; beyond a periodic one lies the other end
        of p when p spans the domain."""
        for d in range(3):
            ax = 2 - d
            n = p.shape[ax]
            nd = (2 ** l) * self.n_cell[d] // a
            at_lo, at_hi = o[d] == 0, o[d] + n == nd
            first, last = np.take(p, [0], axis=ax), np.take(p, [n - 1], axis=ax)
            if self.periodic[d]:
                wrap = at_lo and at_hi
                below, above = (last, first) if wrap else (np.zeros_like(first), np.zeros_like(first))
            else:
                below = np.ones_like(first) if at_lo else np.zeros_like(first)
                above = np.ones_like(first) if at_hi else np.zeros_like(first)
            q = np.concatenate([below, p, above], axis=ax)
            sl = lambda a0, a1: tuple(slice(a0, a1) if x == ax else slice(None) for x in range(3))
            p = q[sl(0, n)] & q[sl(1, n + 1)] & q[sl(2, n + 2)]
        return p

    def _nesting_cells(self, l, lbase, o, shape, a):
        """Amr::grid_places' proper nesting domain [3P] for the tags of level l when level lbase and everything below
        it keep their boxes: the region of level lbase shrunk by one blocking cell, refined and shrunk by another cell
        for every level up to l -- so that each new level fits around the next with a cell to spare.  Returned over
        the cells (of a zones of level l) of the region (o, shape); None when there is nothing to respect (level 0
        covers the domain)."""
        if lbase == 0:
            return None
        assert all(((2 ** lbase) * self.n_cell[d]) % a == 0 for d in range(3))
        bl = self.lev[lbase].box_list()
        olo = [min(b[0][d] for b in bl) // a for d in range(3)]
        ohi = [max(b[1][d] for b in bl) // a for d in range(3)]
        p = np.zeros(tuple(ohi[d] - olo[d] + 1 for d in (2, 1, 0)), dtype=bool)
        for lo, hi in bl:
            p[tuple(slice(lo[d] // a - olo[d], hi[d] // a - olo[d] + 1) for d in (2, 1, 0))] = True
        p = self._erode_cells(p, olo, lbase, a)
        for i in range(lbase + 1, l + 1):
            p = p.repeat(2, axis=0).repeat(2, axis=1).repeat(2, axis=2)
            olo = [2 * x for x in olo]
            p = self._erode_cells(p, olo, i, a)
        out = np.zeros(shape, dtype=bool)
        src = ((tuple(olo), tuple(olo[d] + p.shape[2 - d] - 1 for d in range(3))))
        it = CL.intersect(src, (tuple(o), tuple(o[d] + shape[2 - d] - 1 for d in range(3))))
        if it:
            out[tuple(slice(it[0][d] - o[d], it[1][d] - o[d] + 1) for d in (2, 1, 0))] = \
                p[tuple(slice(it[0][d] - olo[d], it[1][d] - olo[d] + 1) for d in (2, 1, 0))]
        return out

    def tag_boxes(self, l=0, ghosts_filled=False, cover=(), lbase=None, nest=()):
        """New boxes of level l+1 in level-l zones: clustered, buffered tags of level l, also covering `cover`
        (boxes in level-l zones that the new boxes must contain: the footprint of the level above) and the blocking
        cells of and around `nest` (that footprint without buffer: proper nesting), all inside the proper nesting
        domain of a regrid that leaves levels <= lbase (default l) alone.  Buffering and the reduction to
        blocking_factor/2-sized cells run where the tags are (max-pooling); only the reduced arrays go to the host
        for the clustering."""
        import torch.nn.functional as F
        if not ghosts_filled:
            self._fill_ghosts_new(l)
        tags, mask, o = self._tags(l)
        n = self.n_error_buf
        if n > 0:                                               # amr.n_error_buf: a (2n+1)^3 maximum
            tags = F.max_pool3d(tags[None, None], kernel_size=2 * n + 1, stride=1, padding=n)[0, 0]
        shape = tags.shape
        for lo, hi in cover:
            it = CL.intersect((lo, hi), (o, tuple(o[d] + shape[2 - d] - 1 for d in range(3))))
            if it:
                tags[it[0][2] - o[2]:it[1][2] - o[2] + 1, it[0][1] - o[1]:it[1][1] - o[1] + 1, it[0][0] - o[0]:it[1][0] - o[0] + 1] = 1.0
        tags = tags * mask
        a = max(self.blocking_factor // 2, 1)                   # blocking_factor is in zones of level l+1
        assert all(x % a == 0 for x in o) and all(s % a == 0 for s in shape), "level boxes must be multiples of blocking_factor/2"
        if a > 1:                                               # any zone tagged / all zones valid per a^3 cell
            ct = F.max_pool3d(tags[None, None], kernel_size=a, stride=a)[0, 0]
            cm = -F.max_pool3d(-mask[None, None], kernel_size=a, stride=a)[0, 0]
        else:
            ct, cm = tags, mask
        ct = (ct > 0.5).cpu().numpy()
        if self.nranks > 1:
            # buffering and pooling are maxima, so the maximum over the ranks' partial tags commutes with them: only the
            # reduced arrays travel
            ct = np.logical_or.reduce(self.comm.gather_objects(ct))
        oc = tuple(x // a for x in o)
        for lo, hi in nest:                                     # one cell around the footprint of level l+2
            for sh in self._cell_images(l, a):
                it = CL.intersect((tuple(lo[d] // a - 1 + sh[d] for d in range(3)), tuple(hi[d] // a + 1 + sh[d] for d in range(3))),
                                  (oc, tuple(oc[d] + ct.shape[2 - d] - 1 for d in range(3))))
                if it:
                    ct[tuple(slice(it[0][d] - oc[d], it[1][d] - oc[d] + 1) for d in (2, 1, 0))] = True
        if not ct.any():
            return []
        cm = (cm > 0.5).cpu().numpy()
        pn = self._nesting_cells(l, l if lbase is None else lbase, oc, ct.shape, a)
        if pn is not None:
            cm &= pn
            if not (ct & cm).any():
                return []
        # The clustering is a pure function of the reduced arrays: a regrid that finds the tags of the last one (a front that has
        # not crossed a blocking cell since) takes the boxes of the last one instead of 1-2 ms of Berger-Rigoutsos on the host
        max_size = None if self.max_grid_size is None else max(self.max_grid_size // 2, a)
        key = (ct.shape, ct.tobytes(), cm.tobytes(), tuple(o), a, self.grid_eff, max_size)
        memo = self.__dict__.setdefault("_cluster_memo", {})
        hit = memo.get(l)
        if hit is not None and hit[0] == key:
            return list(hit[1])
        out = CL.boxes_from_coarse(ct, cm, o, a, grid_eff=self.grid_eff, max_size=max_size)
        memo[l] = (key, list(out))
        return out

    def tag_box(self, l=0):
        """The one-box form: (lo, hi) in level-l zones or None."""
        bl = self.tag_boxes(l)
        return bl[0] if bl else None

    # ---- Amr::grid_places: new box lists for levels lbase+1.. (at most one level more than now) ------
    def _grid_places(self, lbase=0, alpha=1.0):
        finest = len(self.lev) - 1
        top = min(finest, self.max_level - 1)                   # the finest level that may carry tags
        self._fill_ghosts_new(top, lbase, alpha)
        new = {l: self.boxes[l] for l in range(1, lbase + 1)}   # levels up to lbase keep their boxes
        for l in range(top, lbase - 1, -1):
            cover, nest = [], []
            for lo, hi in new.get(l + 2, []):                   # proper nesting: contain the level above + a buffer
                nest.append((tuple(_coarsen(lo[d]) for d in range(3)), tuple(_coarsen(hi[d]) for d in range(3))))
                cover.append((tuple(_coarsen(lo[d]) - self.n_error_buf for d in range(3)),
                              tuple(_coarsen(hi[d]) + self.n_error_buf for d in range(3))))
            new[l + 1] = self.tag_boxes(l, ghosts_filled=True, cover=cover, lbase=lbase, nest=nest)
        out = []
        for l in range(1, top + 2):
            if not new.get(l):
                break
            out.append(new[l])
        # boxes of level l+1 were placed on the OLD level-l boxes: keep what lies inside the NEW ones
        for i in range(max(lbase, 1), len(out)):
            kept = []
            for b in out[i]:
                for plo, phi in out[i - 1]:
                    it = CL.intersect(b, (tuple(2 * x for x in plo), tuple(2 * x + 1 for x in phi)))
                    if it:
                        kept.append(it)
            if not kept:
                del out[i:]
                break
            out[i] = sorted(kept, key=lambda b: (b[0][2], b[0][1], b[0][0]))
        return out

    # ---- Amr::regrid(lbase): new grids above level lbase, data from the old boxes of a level where they exist,
    #      else interpolated ---------------------------------------------------------------------------------
    def regrid(self, lbase=0, alpha=1.0):
        """Amr::regrid(lbase), then the particle part of Castro::post_regrid (Castro.cpp:2114-2117): Redistribute(lbase).
        True if the grids changed."""
        changed = self._regrid(lbase, alpha)
        if self.tracers is not None and self.tracers.pos is not None:
            self._particles_redistribute(lbase)
        return changed

    def _regrid(self, lbase=0, alpha=1.0):
        new = self._grid_places(lbase, alpha)
        if new == self.boxes[1:]:
            return False
        old_lev = list(self.lev)
        keep = 1                                                # levels below the first changed box list stay as they are
        while keep <= min(len(new), len(self.lev) - 1) and new[keep - 1] == self.boxes[keep]:
            keep += 1
        del self.lev[keep:]
        self._diag_masks, self._diag_tables = {}, {}
        if self.gravity is not None:
            self.gravity.reset(keep)
        for l in range(keep, len(new) + 1):
            parent = self.lev[l - 1]
            if l - 1 >= keep:                                   # a level made in this regrid: its ghost zones are not filled yet
                parent.alpha = 1.0
                parent.fill("S_new_b")
            self._push_level(new[l - 1])
            lev = self.lev[l]
            h = lev.hydro
            if self.nranks > 1:
                self._xrun([("crse_new", b, p, lo, hi, None) for b in lev.boxes for p, (lo, hi) in b.csrc + b.csrc_valid])
                for b in lev.mine:
                    h.cc_interp(b.ctmp, b.cbox, b.S_new_b, b.gbox, b.lo, b.hi, NUM_STATE)
                if l < len(old_lev):
                    ops = []
                    for b in lev.boxes:
                        for ob in old_lev[l].boxes:
                            it = CL.intersect(ob.bx, b.bx)
                            if it:
                                ops.append(("copy", b, ob, it[0], it[1], ("S_new_b", (0, 0, 0))))
                    self._xrun(ops)
                lev.time, lev.nstep = self.time, self.nstep
                continue
            for b in lev.boxes:
                # FillCoarsePatch: cell-conservative interpolation of the (ghost-filled) coarse data over the whole new box
                for p, (lo, hi) in b.csrc + b.csrc_valid:
                    h.lincomb(b.ctmp, b.cbox, 0.0, p.S_new_b, p.gbox, 1.0, p.S_new_b, p.gbox, NUM_STATE, lo, hi)
                h.cc_interp(b.ctmp, b.cbox, b.S_new_b, b.gbox, b.lo, b.hi, NUM_STATE)
                if l < len(old_lev):
                    for ob in old_lev[l].boxes:
                        it = CL.intersect(ob.bx, b.bx)
                        if it:
                            h.copy(b.S_new_b, b.gbox, ob.S_new_b, ob.gbox, it[0], it[1])
            lev.time, lev.nstep = self.time, self.nstep
        self.nregrid += 1
        return True

    # ---- Amr::init (bldFineLevels: one new level per pass) / Castro::post_init ---------------------------
    def initData(self, problem="sedov", **kw):
        self.invalidate_estimates()                     # also on an existing hierarchy: no estimate survives new data
        for b in self.lev[0].mine:
            b.initData(problem, **kw)
        if self.refine is not None:
            self._drop_fine()
            while len(self.lev) - 1 < self.max_level:
                bl = self.tag_boxes(len(self.lev) - 1)
                if not bl:
                    break
                self._push_level(bl)
                for b in self.lev[-1].mine:
                    b.initData(problem, **kw)                   # fine levels start from the problem initialiser
            # Amr::bldFineLevels' closing loop [3P]: each level above was placed inside the one before it; regrid from
            # level 0 (initial data from the initialiser again) until the coarser levels have grown around the finer
            # ones and the box lists stay as they are
            for _ in range(4):
                if len(self.lev) == 1:
                    break
                for l in range(len(self.lev) - 1, 0, -1):
                    self.avgDown(l)
                new = self._grid_places(0)
                if new == self.boxes[1:]:
                    break
                self._drop_fine()
                for bl in new:
                    self._push_level(bl)
                    for b in self.lev[-1].mine:
                        b.initData(problem, **kw)
        else:
            for lev in self.lev[1:]:
                for b in lev.mine:
                    b.initData(problem, **kw)
        # Castro::post_init (Castro.cpp:2220-2235): average down from the finest level, nothing else -- the averaged zones
        # are first cleaned by initialize_advance
        for l in range(len(self.lev) - 1, 0, -1):
            self.avgDown(l)
        self.time, self.nstep = 0.0, 0
        self.level_count = [0] * 16
        if self.tracers is not None:                    # Castro::init_particles on level 0, Redistribute(0) over the built levels
            self.tracers.init_particles(self.lev[0].geom)
            self._particles_redistribute(0)
            self.tracers.check_flags()
        self.diag.reset()
        if self.diag.sum_interval > 0:                  # Castro::post_init: the entry of time 0, dt reported as 0
            self.diag.record(self.sum_integrated_quantities(), 0, 0.0, finest_level=len(self.lev) - 1)

    # ---- tracer particles over the hierarchy (castro_amd/particles.py) ---------------------------------------------------
    def _tracer_levels(self):
        return [lev.box_list() for lev in self.lev], [lev.geom for lev in self.lev]

    def _particles_redistribute(self, lev_min, ngrow=0):
        boxes, geoms = self._tracer_levels()
        owners = [[b.owner for b in lev.boxes] for lev in self.lev] if self.nranks > 1 else None
        self.tracers.redistribute(boxes, geoms, lev_min, len(self.lev) - 1, ngrow, owners=owners)

    def _particles_post_timestep(self, l, iteration, t_new, alpha_new):
        """the particle part of Castro::post_timestep of level l (Castro.cpp:1982-1997), under the reference's condition
        `iteration < ncycle || level == 0` -- not after the last of a refined level's two subcycles, whose particles the coarser
        level's call covers: Redistribute(l, finest, ngrow = 0 on level 0, else the iteration) and TimestampParticles(ngrow + 1)
        over the levels from l up, whose new-time ghost zones are filled for it (level l sits at alpha_new inside its parent's
        step)."""
        tr = self.tracers
        if tr is None or (l > 0 and iteration >= 2):
            return
        self._particles_redistribute(l, 0 if l == 0 else iteration)
        if tr.timestamp_dir is not None:
            keep = [lev.alpha for lev in self.lev]
            self._fill_ghosts_new(len(self.lev) - 1, l, alpha_new)      # ghost zones only: the run does not change
            for lev, a in zip(self.lev, keep):
                lev.alpha = a
            tr.timestamp(l, t_new, lambda k: self.lev[k]._tracer_boxes("S_new_b"), self._tracer_levels()[1])

    def writePlotFile(self, dirname, derive=None):
        from .plotfile import write_plotfile_amr
        return write_plotfile_amr(dirname, self, derive=derive)

    # ---- Castro::avgDown (Castro.cpp:3096-3113): level l onto level l-1 ------------------------------
    def invalidate_estimates(self):
        """call after writing any level's S_new from outside (user edits between coarse steps): see _Level.invalidate_estimate"""
        for lev in self.lev:
            lev.invalidate_estimate()

    def avgDown(self, l=1):
        self.lev[l - 1].invalidate_estimate()           # the coarser level's S_new is overwritten under the fine boxes
        if self.nranks > 1:
            return self._xrun([("avgdown", p, b, lo, hi, None) for b in self.lev[l].boxes for p, (lo, hi) in b.avg_to])
        fine = self.lev[l]
        h = fine.hydro
        if fine._level_calls():
            # the whole level in one launch (CASTRO_AMD_OP_AVGDOWN): the regions are disjoint zones of the coarse level
            pp = tuple(b.S_new_b.data_ptr() for b in fine.boxes) + tuple(p.S_new_b.data_ptr() for p in self.lev[l - 1].boxes)
            h.fab_ops(fine._cached_ops(("avgdown",), pp, lambda: h.make_ops(
                [(L.OP_AVGDOWN, 0, NUM_STATE, lo, hi, 0.0, 0.0, (p.S_new_b, p.gbox), (b.S_new_b, b.gbox), None)
                 for b in fine.boxes for p, (lo, hi) in b.avg_to])), params=fine.params)
            return
        for b in fine.boxes:
            for p, (lo, hi) in b.avg_to:
                h.avgdown(b.S_new_b, b.gbox, p.S_new_b, p.gbox, lo, hi, NUM_STATE)

    # ---- Castro::computeInitialDt / computeNewDt over the hierarchy ----------------------------------
    def _dt0(self, stop_time, initial):
        P = self.params
        n_factor, dt_0 = 1, 1.e100
        for l, lev in enumerate(self.lev):
            n_factor *= (1 if l == 0 else 2)
            dt = lev.estTimeStep()
            if initial:
                dt *= P.init_shrink
            else:
                dt = min(dt, P.change_max * self.dt_level[l])
            dt_0 = min(dt_0, n_factor * dt)
        if initial:
            eps = 0.001 * dt_0
            if stop_time >= 0.0 and (self.time + dt_0) > (stop_time - eps):
                dt_0 = stop_time - self.time
        else:
            eps = 2.220446049250313e-16
            if stop_time >= 0.0 and (self.time + dt_0) >= (stop_time - eps):
                dt_0 = stop_time - self.time
        return dt_0

    # ---- Amr::timeStep: advance level l, then recursively twice the next finer level, then post_timestep -----
    def _time_step(self, l, t, dt, alpha, iteration=1):
        """alpha: position of this level's old time inside the parent's [old, new] interval (0 or 1/2); iteration: which of the
        parent's subcycles this is (1 on level 0, 1 or 2 above)."""
        # Amr::timeStep: every level i >= l that has taken regrid_int steps since its last regrid gets new grids above
        # it (all those levels are synchronised at time t here)
        if self.refine is not None and self.regrid_int > 0:
            i = l
            while i <= min(len(self.lev) - 1, self.max_level - 1):
                if self.level_count[i] >= self.regrid_int:
                    self.regrid(i, alpha if i == l else 1.0)
                    for k in range(i, len(self.level_count)):
                        self.level_count[k] = 0
                i += 1
        lev, finest = self.lev[l], len(self.lev) - 1
        h = lev.hydro
        lev.alpha = alpha
        lev._t0, lev._alpha0, lev._dt_parent = t, alpha, 2.0 * dt
        lev.t_old, lev.t_new = t, t + dt        # StateData::prevTime / curTime of the level (Gravity::make_radial_gravity)
        lev.fuse_post_level = l == finest and os.environ.get("CASTRO_AMD_FUSE_POST_FINEST", "1") != "0"
        lev._iteration = iteration
        lev.advance(t, dt)
        self.level_count[l] += 1
        if l > 0:
            # FluxRegFineAdd: + this level's fluxes (already dt x area) summed over the 4 fine faces
            if lev.batched:
                h.fab_ops(lev.ops_fine_add)
            else:
                for b in lev.mine:
                    for (d, side), (reg, rbox) in b.regs.items():
                        h.fluxreg_fine_add(reg, rbox, b.fluxes[d], b.flux_boxes[d], rbox[0], rbox[1], d, NUM_STATE, 1.0)
        if l < finest:
            fine = self.lev[l + 1]
            # ghost zones of the new data of this level, for the FillPatch of the next finer one
            lev.alpha = alpha + 0.5
            lev.fill("S_new_b")
            if lev.have_sources:
                lev.fill_new_source()
            # FluxRegCrseInit: -1 x this level's fluxes through the faces of the finer boxes
            if self.nranks > 1:
                self._xrun([("crse_init", b, p, lo, hi, (d, side)) for b in fine.boxes for (d, side) in b.regs
                            for p, (lo, hi) in b.crse_init[(d, side)]])
            elif fine.batched:
                h.fab_ops(fine.ops_crse_init)
            else:
                for b in fine.boxes:
                    for (d, side), (reg, rbox) in b.regs.items():
                        for p, (lo, hi) in b.crse_init[(d, side)]:
                            h.fluxreg_crse_init(reg, rbox, p.fluxes[d], p.flux_boxes[d], lo, hi, NUM_STATE, -1.0)
            for it in range(2):
                self._time_step(l + 1, t + it * (dt / 2), dt / 2, 0.5 * it, iteration=it + 1)
            # post_timestep: reflux, avgDown, clean_state
            vol = lev.geom.dx[0] * lev.geom.dx[1] * lev.geom.dx[2]
            # face orientation by face orientation, like FluxRegister::Reflux's OrientationIter [3P]: the registers of one
            # orientation touch disjoint coarse zones (two boxes with a common outside neighbour on the same side would
            # overlap), so they can share launches; a zone next to several boxes gets its contributions in this order
            if self.nranks > 1:
                self._xrun([("reflux", p, b, lo, hi, (d, side, vol, csh)) for d in range(3) for side in (0, 1)
                            for b in fine.boxes for p, (lo, hi), csh in b.reflux_to[(d, side)]])
            for d in (range(3) if self.nranks == 1 else ()):
                for side in (0, 1):
                    if fine.batched:
                        pp = tuple(p.S_new_b.data_ptr() for p in lev.boxes)
                        h.fab_ops(fine._cached_ops(("reflux", d, side), pp, lambda d=d, side=side: h.make_ops(
                            [(L.OP_REFLUX, (d, side), NUM_STATE, lo, hi, vol, 0.0, (p.S_new_b, _shift(p.gbox, csh)), b.regs[(d, side)], None)
                             for b in fine.boxes for p, (lo, hi), csh in b.reflux_to[(d, side)]])))
                    else:
                        for b in fine.boxes:
                            reg, rbox = b.regs[(d, side)]
                            for p, (lo, hi), csh in b.reflux_to[(d, side)]:
                                h.reflux(p.S_new_b, _shift(p.gbox, csh), reg, rbox, lo, hi, d, side, NUM_STATE, vol)
            lev.invalidate_estimate()                   # reflux has corrected this level's S_new
            if self.update_sources_after_reflux:
                self._fluxes_after_reflux(l)
                for k in (l + 1, l):                    # the finer level first (Castro.cpp:2777)
                    self.lev[k].renew_sources()
            self.avgDown(l + 1)
        # Castro::post_timestep ends with clean_state(S_new) on EVERY level (Castro.cpp:1909-1916), the finest included
        # (there it may have ridden in the fused pass of the update: _hydro_level)
        if not (l == finest and lev._post_clean_done):
            lev.clean_new()
        self._particles_post_timestep(l, iteration, t + dt, alpha + 0.5)

    def _fluxes_after_reflux(self, l):
        """Castro::reflux with castro.update_sources_after_reflux, the flux half (Castro.cpp:2617-2644): the registers of level
        l + 1 are added to the fluxes of level l on the faces of the coarse-fine boundary, the mass fluxes take the density
        component there -- and on the whole level where fluxes and mass fluxes differ (after retry subcycles the fluxes are sums
        over the subcycles, the mass fluxes those of the last one).  Whether or not the level has sources."""
        lev, fine = self.lev[l], self.lev[l + 1]
        h = lev.hydro
        if self.nranks > 1:
            self._xrun([("reg_to_flux", p, b, lo, hi, (d, side, csh)) for d in range(3) for side in (0, 1)
                        for b in fine.boxes for p, (lo, hi), csh in b.flux_to[(d, side)]])
        for d in (range(3) if self.nranks == 1 else ()):
            for side in (0, 1):                         # the faces of one orientation are disjoint: one launch
                if fine.batched:
                    h.fab_ops(fine._cached_ops(("reg_to_flux", d, side), (), lambda d=d, side=side: h.make_ops(
                        [(L.OP_FLUXREG_TO_FLUX, d, NUM_STATE, lo, hi, 0.0, 0.0, (p.fluxes[d], _shift(p.flux_boxes[d], csh)),
                          b.regs[(d, side)], (p.mass_fluxes[d], _shift(p.flux_boxes[d], csh)))
                         for b in fine.boxes for p, (lo, hi), csh in b.flux_to[(d, side)]])))
                else:
                    for b in fine.boxes:
                        reg, rbox = b.regs[(d, side)]
                        for p, (lo, hi), csh in b.flux_to[(d, side)]:
                            fbox = _shift(p.flux_boxes[d], csh)
                            h.fluxreg_to_flux(p.fluxes[d], fbox, reg, rbox, p.mass_fluxes[d], fbox, lo, hi, NUM_STATE)
        if lev.nsubcycles > 1:
            for p in lev.mine:
                for d in range(3):
                    fb = p.flux_boxes[d]
                    h.copy(p.mass_fluxes[d], fb, p.fluxes[d][0:1], fb, fb[0], fb[1])

    # ---- Amr::coarseTimeStep ---------------------------------------------------------------------
    def step(self, stop_time=-1.0):
        self.diag.begin_steps(1)
        dt0 = self._dt0(stop_time, self.nstep == 0)
        for l in range(len(self.dt_level)):
            self.dt_level[l] = dt0 / (2 ** l)
        t = self.time
        self._time_step(0, t, dt0, 0.0)
        self.time = t + dt0
        self.nstep += 1
        for lev in self.lev:
            lev.time, lev.nstep = self.time, self.nstep
        if self.tracers is not None:
            self.tracers.check_flags()                  # the step's one look at the clamp and lost counts
        if self.diag.due(self.nstep):                   # Castro::post_timestep of level 0
            self.diag.record(self.sum_integrated_quantities(), self.nstep, dt0, finest_level=len(self.lev) - 1)
        return dt0

    def evolve(self, stop_time, max_step=10 ** 9):
        eps = 2.220446049250313e-16
        while self.nstep < max_step and self.time < stop_time - eps:
            self.step(stop_time)
            self._checkpoint_post_timestep()    # amr.check_int: nstep % check_int == 0, written in the background
        return self.nstep

    def close(self):
        """join a checkpoint in flight and re-raise what its thread raised (collective on more than one rank); with Poisson
        gravity, give back the multigrid plans of the levels (a later step makes them again)"""
        self.checkpoint_wait()
        if hasattr(getattr(self, "gravity", None), "close"):
            self.gravity.close()

    def __del__(self):
        try:
            self._checkpoint_join_only()        # a finaliser issues no collective and raises nothing: the thread only
        except Exception:
            pass

    # ---- diagnostics -------------------------------------------------------------------------
    def composite_sum(self, comp):
        """Volume integral of a conserved component over the composite grid (finest data wherever refined)."""
        tot = 0.0
        for l, lev in enumerate(self.lev):
            v = lev.geom.dx[0] * lev.geom.dx[1] * lev.geom.dx[2]
            for b in lev.boxes:
                S = b.S_new()[comp]
                if l + 1 < len(self.lev):
                    S = S.clone()
                    o = b.lo
                    for f in self.lev[l + 1].boxes:
                        it = CL.intersect(f.pbox, b.bx)
                        if it:
                            (p, q) = it
                            S[p[2] - o[2]:q[2] - o[2] + 1, p[1] - o[1]:q[1] - o[1] + 1, p[0] - o[0]:q[0] - o[0] + 1] = 0.0
                tot += S.sum().item() * v
        return tot

    # ---- Castro::sum_integrated_quantities over the hierarchy (Source/driver/sum_integrated_quantities.cpp:60-120) ----------
    sum_interval = property(lambda self: self.diag.sum_interval)
    diag_history = property(lambda self: self.diag.history)

    def _diag_mask_key(self, l):
        """what the byte masks of level l depend on: its own boxes and the coarse zones the next level covers"""
        return (tuple(self.lev[l].box_list()), tuple(tuple(map(tuple, f.pbox)) for f in self.lev[l + 1].boxes))

    def _diag_level_masks(self, l):
        """{box: uint8 tensor (nz, ny, nx), 0 where level l + 1 covers the zone} for the boxes of level l this rank owns (the
        build_fine_mask of sum_utils.cpp:29-33); None for the finest level.  Built once per regrid: regrid, _push_level and
        _drop_fine empty the cache."""
        if l + 1 >= len(self.lev):
            return None
        cache = self.__dict__.setdefault("_diag_masks", {})
        key = self._diag_mask_key(l)
        ent = cache.get(l)
        if ent is None or ent[0] != key:
            masks = {}
            for b in self.lev[l].mine:
                m = torch.ones((b.n[2], b.n[1], b.n[0]), dtype=torch.uint8, device=b.S_new_b.device)
                o = b.lo
                for f in self.lev[l + 1].boxes:
                    it = CL.intersect(f.pbox, b.bx)
                    if it:
                        (p, q) = it
                        m[p[2] - o[2]:q[2] - o[2] + 1, p[1] - o[1]:q[1] - o[1] + 1, p[0] - o[0]:q[0] - o[0] + 1] = 0
                masks[b.bx] = m
            ent = cache[l] = (key, masks)
        return ent[1]

    def sum_integrated_quantities(self):
        """The integrated quantities of the composite grid (the finest data wherever a zone is refined): one library call per
        level -- below the finest with the byte masks of the zones the next level covers --, the 14-vectors of the levels
        added on the device in level order, then one allreduce(SUM) and one copy to the host for the whole hierarchy."""
        from . import diag
        center = diag.domain_center(self.lev[0])
        tot = None
        for l, lev in enumerate(self.lev):
            h = lev.hydro
            if not hasattr(h, "integrated_quantities_mf"):
                raise RuntimeError("castro_amd: this backend has no integrated_quantities_mf; there is no host fallback")
            if self._diag_out is None:
                self._diag_out = [h.alloc(1, (0, 0, 0), (L.DIAG_N - 1, 0, 0)).reshape(L.DIAG_N) for _ in range(2)]
            masks = self._diag_level_masks(l)
            sp = tuple(b.S_new_b.data_ptr() for b in lev.mine) + tuple(m.data_ptr() for m in (masks or {}).values())
            tables = self.__dict__.setdefault("_diag_tables", {})     # raw pointers: one table per configuration of the state buffers
            if (l, sp) not in tables:
                if len(tables) > 64:
                    tables.clear()
                tables[(l, sp)] = h.make_diag_boxes(
                    [(b.lo, b.hi, (b.S_new_b, b.gbox), masks[b.bx] if masks is not None else None) for b in lev.mine])
            boxes = tables[(l, sp)]
            out = self._diag_out[0 if l == 0 else 1]
            h.integrated_quantities_mf(boxes, lev.geom, center, out)
            if l == 0:
                tot = out
            else:
                tot += out
        self.comm.allreduce_sum(tot)
        return diag.quantities(self.time, tot.tolist())

    def zones_advanced_per_coarse_step(self):
        """Zone updates of one coarse step (level l advances 2^l times): the reference's FOM numerator."""
        return sum((2 ** l) * sum(b.n[0] * b.n[1] * b.n[2] for b in lev.boxes) for l, lev in enumerate(self.lev))

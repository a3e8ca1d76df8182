"""Host-side mirror of the reference's hydro interface over the C ABI.

`HipHydro` is the per-(device, stream) object whose methods carry the reference's names
(`construct_ctu_hydro_source`, `clean_state`, `estdt_cfl`, ...) and take FABs as torch CUDA
tensors shaped (ncomp, nz, ny, nx) plus their index box.  torch is used for device
memory and streams only; every operation is a call into libcastro_hydro_amd.so.
"""
import ctypes as C

import torch

from . import _lib as L


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr(stream):
    """hipStream_t of `stream`, or of torch's current stream on the current device (the raw-handle query is ~20x cheaper
    than torch.cuda.current_stream(), which matters when a level of small boxes issues thousands of calls per step)."""
    if stream is None:
        if _raw_stream is not None:
            return C.c_void_p(_raw_stream(torch.cuda.current_device()))
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


class HipHydro:
    """One castro_amd_ctx.  No CPU fallback: constructing it without a HIP device raises."""

    name = "hip"

    def __init__(self, device=0, numerics=None):
        """numerics: "exact" | "contract" (None: CASTRO_AMD_NUMERICS, default exact) -- which build of the kernel library
        this context runs (castro_amd/_lib.py)."""
        if not torch.cuda.is_available():
            raise RuntimeError("castro_amd.HipHydro needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = L.load(numerics)
        self.numerics = L.numerics_of(self.lib)
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        L.check(self.lib.castro_amd_ctx_create(C.byref(h), int(device)), "ctx_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.castro_amd_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            # a finaliser that runs in the middle of a stream capture must not free device memory (the runtime aborts):
            # leave the context to the end of the process instead
            if torch.cuda.is_current_stream_capturing():
                return
            self.close()
        except Exception:
            pass

    # ---- memory -------------------------------------------------------------------------
    def alloc(self, ncomp, lo, hi, fill=0.0):
        """A FAB for box [lo,hi] as a torch tensor (ncomp, nz, ny, nx), FP64, on the device."""
        shape = (ncomp, hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
        return torch.full(shape, fill, dtype=torch.float64, device=self.device)

    def reserve(self, nx, ny, nz):
        L.check(self.lib.castro_amd_ctx_reserve(self.h, nx, ny, nz), "ctx_reserve")

    def scratch_bytes(self):
        return int(self.lib.castro_amd_ctx_scratch_bytes(self.h))

    def status(self, stream=None):
        return int(self.lib.castro_amd_ctx_status(self.h, _stream_ptr(stream)))

    def set_source_corrector(self, corr, box):
        """Castro::source_corrector for the hydro calls that follow (params.source_term_predictor = 1); None clears it."""
        fab = L.fab_of(corr, *box) if corr is not None else L.fab_desc(None, (0, 0, 0), (0, 0, 0), 0)
        L.check(self.lib.castro_amd_ctx_set_source_corrector(self.h, C.byref(fab)), "ctx_set_source_corrector")

    def poison_scratch(self, stream=None):
        """NaN-fill the scratch arena (tests: a call must not read what an earlier call left there)."""
        L.check(self.lib.castro_amd_ctx_poison_scratch(self.h, _stream_ptr(stream)), "ctx_poison_scratch")

    # ---- pointwise forms (known-answer vectors at the level of the reference's own functions) ----
    def cmpflx_points(self, idir, qm, qp, cl, cr, params, bnd_fac=None, is_shock=None):
        """Castro::cmpflx_plus_godunov's body on n interfaces: qm, qp (7, n); returns (11, n)."""
        n = qm.shape[1]
        out = torch.empty((11, n), dtype=torch.float64, device=self.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        L.check(self.lib.castro_amd_cmpflx_points(n, int(idir), ptr(qm), ptr(qp), ptr(cl), ptr(cr), ptr(bnd_fac), ptr(is_shock),
                                                  C.byref(params), ptr(out), _stream_ptr(None)), "cmpflx_points")
        return out

    def ppm_points(self, s, flatn, u, c, dtdx):
        """ppm_reconstruct + ppm_int_profile: s (5, n) -> (sm, sp, Ip[3], Im[3]) as (8, n)."""
        n = s.shape[1]
        out = torch.empty((8, n), dtype=torch.float64, device=self.device)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        L.check(self.lib.castro_amd_ppm_points(n, ptr(s), ptr(flatn), ptr(u), ptr(c), float(dtdx), ptr(out), _stream_ptr(None)),
                "ppm_points")
        return out

    def flatten_points(self, p7, u5):
        n = p7.shape[1]
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        L.check(self.lib.castro_amd_flatten_points(n, ptr(p7), ptr(u5), ptr(out), _stream_ptr(None)), "flatten_points")
        return out

    def trans_points(self, q, f1r, f1l, cdtdx1, params, tdir=0, f2r=None, f2l=None, cdtdx2=0.0, fe=None):
        """actual_trans_single (f2r is None) / actual_trans_final: q (7, n), flux records (8, n) -> (7, n);
        fe: (2 or 4, n) (rho e) fluxes for transverse_reset_rhoe = 1."""
        n = q.shape[1]
        out = torch.empty((7, n), dtype=torch.float64, device=self.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        L.check(self.lib.castro_amd_trans_points(n, 2 if f2r is not None else 1, int(tdir), ptr(q), ptr(f1r), ptr(f1l), ptr(f2r),
                                                 ptr(f2l), ptr(fe), float(cdtdx1), float(cdtdx2), C.byref(params), ptr(out),
                                                 _stream_ptr(None)), "trans_points")
        return out

    # ---- the hot path: Castro::construct_ctu_hydro_source, one FAB/tile --------------------
    def construct_ctu_hydro_source(self, bx, Sborder, sb_box, S_new, snew_box, geom, params, time, dt,
                                   fluxes=None, flux_boxes=None, mass_fluxes=None, qe=None, vbx=None,
                                   update_from_sborder=False, src=None, src_box=None, stream=None,
                                   clean_ntimes=0, red=None, flux_assign=False, stage=None, sborder_clean=0, d_dt=None, bc_fill=False):
        """clean_ntimes > 0 selects castro_amd_ctu_hydro_clean_fab: the update is followed, in the same
        pass, by S_new.min(URHO), clean_state x clean_ntimes and the CFL estimate, reduced into `red`.
        sborder_clean > 0 (castro_amd_ctu_hydro_fab_ex): clean_state that many times on every zone of Sborder, in place,
        inside the pass that reads it.  d_dt: a device tensor whose first element is the time step (host-free stepping;
        `dt` is ignored)."""
        bxlo, bxhi = bx
        vlo, vhi = vbx if vbx is not None else bx
        fb = (L.Fab * 3)()
        mb = (L.Fab * 3)()
        qb = (L.Fab * 3)()
        for d in range(3):
            if flux_boxes is not None:
                flo, fhi = flux_boxes[d]
            else:
                flo, fhi = list(vlo), list(vhi)
                fhi[d] += 1
            fb[d] = L.fab_of(fluxes[d] if fluxes is not None else None, flo, fhi)
            mb[d] = L.fab_of(mass_fluxes[d] if mass_fluxes is not None else None, flo, fhi)
            qb[d] = L.fab_of(qe[d] if qe is not None else None, flo, fhi)
        sfab = L.fab_of(src, *src_box) if src is not None else L.fab_desc(None, bxlo, bxhi, 0)
        flags = L.UPDATE_FROM_SBORDER if update_from_sborder else L.UPDATE_ADD
        if flux_assign:
            flags |= L.FLUX_ASSIGN
        if stage is not None:         # "A": the ghost-free part (overlaps the halo exchange); "B": the rest -- the round-2 split;
            #                           "valid": ctoprim (+ the cleans) on the valid zones only; "rest": everything else (round 6)
            flags |= {"A": L.STAGE_A, "B": L.STAGE_B, "valid": L.STAGE_VALID, "rest": L.STAGE_REST}[stage]
        if bc_fill:                   # the call fills the physical-boundary zones of Sborder itself (CASTRO_AMD_BC_FILL)
            flags |= L.BC_FILL
        if sborder_clean > 0 or d_dt is not None:
            o = L.HydroOpts(flags, int(clean_ntimes), red.data_ptr() if red is not None else None, int(sborder_clean),
                            d_dt.data_ptr() if d_dt is not None else None)
            rc = self.lib.castro_amd_ctu_hydro_fab_ex(
                self.h, L.i3(bxlo), L.i3(bxhi), L.i3(vlo), L.i3(vhi),
                C.byref(L.fab_of(Sborder, *sb_box)), C.byref(sfab), C.byref(L.fab_of(S_new, *snew_box)),
                fb, mb, qb, C.byref(geom), C.byref(params), float(time), float(dt), C.byref(o), _stream_ptr(stream))
            L.check(rc, "ctu_hydro_fab_ex")
            return
        if clean_ntimes > 0:
            rc = self.lib.castro_amd_ctu_hydro_clean_fab(
                self.h, L.i3(bxlo), L.i3(bxhi), L.i3(vlo), L.i3(vhi),
                C.byref(L.fab_of(Sborder, *sb_box)), C.byref(sfab), C.byref(L.fab_of(S_new, *snew_box)),
                fb, mb, qb, C.byref(geom), C.byref(params), float(time), float(dt), flags,
                int(clean_ntimes), C.c_void_p(red.data_ptr()) if red is not None else None, _stream_ptr(stream))
            L.check(rc, "ctu_hydro_clean_fab")
            return
        rc = self.lib.castro_amd_ctu_hydro_fab(
            self.h, L.i3(bxlo), L.i3(bxhi), L.i3(vlo), L.i3(vhi),
            C.byref(L.fab_of(Sborder, *sb_box)), C.byref(sfab), C.byref(L.fab_of(S_new, *snew_box)),
            fb, mb, qb, C.byref(geom), C.byref(params), float(time), float(dt), flags, _stream_ptr(stream))
        L.check(rc, "ctu_hydro_fab")

    # ---- gravity source terms (Source/gravity/Castro_gravity.cpp) and apply_source_to_state ----------
    def old_gravity_source(self, state, box, source, src_box, lo, hi, grav, grav_source_type, dt, stream=None):
        g = (C.c_double * 3)(*[float(x) for x in grav])
        L.check(self.lib.castro_amd_old_gravity_source_fab(self.h, C.byref(L.fab_of(state, *box)), C.byref(L.fab_of(source, *src_box)),
                                                           L.i3(lo), L.i3(hi), C.byref(g), int(grav_source_type), float(dt),
                                                           _stream_ptr(stream)), "old_gravity_source_fab")

    def new_gravity_source(self, state_old, old_box, state_new, new_box, source, src_box, mass_fluxes, flux_boxes, lo, hi,
                           grav, grav_source_type, dt, geom, stream=None):
        g = (C.c_double * 3)(*[float(x) for x in grav])
        mb = (L.Fab * 3)()
        for d in range(3):
            mb[d] = L.fab_of(mass_fluxes[d], *flux_boxes[d])
        L.check(self.lib.castro_amd_new_gravity_source_fab(self.h, C.byref(L.fab_of(state_old, *old_box)),
                                                           C.byref(L.fab_of(state_new, *new_box)),
                                                           C.byref(L.fab_of(source, *src_box)), mb, L.i3(lo), L.i3(hi), C.byref(g),
                                                           int(grav_source_type), float(dt), C.byref(geom), _stream_ptr(stream)),
                "new_gravity_source_fab")

    # ---- monopole gravity (Source/gravity/Gravity.cpp) and the gravity sources with a per-zone vector -------------------
    def radial_mass_mf(self, boxes, geom, mono, out, stream=None):
        """castro_amd_radial_mass_mf: Gravity::compute_radial_mass over the valid zones of `boxes` (make_diag_boxes) into `out`, a
        device tensor of 2 * n1d doubles (mass, then volume), overwritten.  Deterministic: the same boxes give the same bits."""
        arr, n = boxes
        L.check(self.lib.castro_amd_radial_mass_mf(self.h, n, arr, C.byref(geom), C.byref(mono), C.c_void_p(out.data_ptr()),
                                                   _stream_ptr(stream)), "radial_mass_mf")

    def radial_gravity(self, mono, geom, mass_vol, radial_grav, stream=None):
        """castro_amd_radial_gravity: the outward integration of make_radial_gravity, mass_vol (2 * n1d) -> radial_grav (n1d)"""
        L.check(self.lib.castro_amd_radial_gravity(self.h, C.byref(mono), C.byref(geom), C.c_void_p(mass_vol.data_ptr()),
                                                   C.c_void_p(radial_grav.data_ptr()), _stream_ptr(stream)), "radial_gravity")

    def monopole_grav(self, radial_grav, mono, geom, grav, grav_box, stream=None):
        """castro_amd_monopole_grav_fab: interpolate_monopole_grav onto the whole box of the 3-component FAB `grav`"""
        L.check(self.lib.castro_amd_monopole_grav_fab(self.h, C.c_void_p(radial_grav.data_ptr()), C.byref(mono), C.byref(geom),
                                                      C.byref(L.fab_of(grav, *grav_box)), _stream_ptr(stream)), "monopole_grav_fab")

    @staticmethod
    def make_radial_boxes(specs):
        """ctypes array of castro_amd_radial_box from (lo, hi, (S_old, box), (S_new, box), mask) -- mask as in make_diag_boxes; the
        weights are set per call (radial_mass_mf_ex)."""
        arr = (L.RadialBox * max(len(specs), 1))()
        keep = []
        for rb, (lo, hi, so, sn, mask) in zip(arr, specs):
            for d in range(3):
                rb.lo[d], rb.hi[d] = lo[d], hi[d]
            rb.state_old, rb.state_new = L.fab_of(so[0], *so[1]), L.fab_of(sn[0], *sn[1])
            if mask is not None:
                shape = (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
                if mask.dtype != torch.uint8 or tuple(mask.shape) != shape or not mask.is_contiguous():
                    raise AssertionError("a mask is a contiguous uint8 tensor shaped (nz, ny, nx) of its box: %s %s for %s"
                                         % (mask.dtype, tuple(mask.shape), shape))
                rb.mask = mask.data_ptr()
                keep.append(mask)
        arr._masks = keep
        return arr, len(specs)

    def radial_mass_mf_ex(self, boxes, omalpha, alpha, geom, mono, out, stream=None):
        """castro_amd_radial_mass_mf_ex: radial_mass_mf over rho = (rho_old * omalpha) + (rho_new * alpha) of `boxes`
        (make_radial_boxes): a coarser level between its two time levels (Gravity.cpp:2987-3000)"""
        arr, n = boxes
        for i in range(n):
            arr[i].omalpha, arr[i].alpha = float(omalpha), float(alpha)
        L.check(self.lib.castro_amd_radial_mass_mf_ex(self.h, n, arr, C.byref(geom), C.byref(mono), C.c_void_p(out.data_ptr()),
                                                      _stream_ptr(stream)), "radial_mass_mf_ex")

    def radial_combine(self, level, mass_vols, n1ds, out, stream=None):
        """castro_amd_radial_combine: radial_mass_summed / radial_vol_summed of `level` from the arrays of levels 0 .. level
        (device tensors of 2 * n1ds[lev] doubles, summed over the ranks) into `out` (2 * n1ds[level])"""
        ptrs = (C.c_void_p * (level + 1))(*[t.data_ptr() for t in mass_vols[:level + 1]])
        ns = (C.c_int * (level + 1))(*[int(x) for x in n1ds[:level + 1]])
        L.check(self.lib.castro_amd_radial_combine(self.h, int(level), ptrs, ns, C.c_void_p(out.data_ptr()), _stream_ptr(stream)),
                "radial_combine")

    def grav_bc_fill(self, grav, grav_box, geom, stream=None):
        """castro_amd_grav_bc_fill_fab: the Gravity_Type boundary fill of the zones of `grav` (3 components) outside the domain"""
        L.check(self.lib.castro_amd_grav_bc_fill_fab(self.h, C.byref(L.fab_of(grav, *grav_box)), C.byref(geom), _stream_ptr(stream)),
                "grav_bc_fill_fab")

    @staticmethod
    def make_grav_fabs(specs):
        """ctypes array of castro_amd_fab from (grav, box): the grav_old or grav_new FABs of the boxes of a sources_mf_g call"""
        arr = (L.Fab * max(len(specs), 1))()
        for i, (g, box) in enumerate(specs):
            arr[i] = L.fab_of(g, *box)
        return arr

    # ---- Poisson gravity on a single level (Source/gravity/Gravity.cpp; castro_amd/csrc/poisson_kernels.hip) ---------------
    def multipole_moments_mf(self, boxes, geom, mp, out, stream=None):
        """castro_amd_multipole_moments_mf: qL0, qLC, qLS of the density over the valid zones of `boxes` (make_diag_boxes) into
        `out`, a device tensor of 3 * (lnum + 1)**2 doubles ([kind][l][m]), overwritten.  The same boxes give the same bits
        (calls of one context on different streams must be ordered by the host: one workspace).  A zone centred exactly on
        mp.center gives NaN for l >= 1, as in the reference."""
        arr, n = boxes
        L.check(self.lib.castro_amd_multipole_moments_mf(self.h, n, arr, C.byref(geom), C.byref(mp), C.c_void_p(out.data_ptr()),
                                                         _stream_ptr(stream)), "multipole_moments_mf")

    def multipole_phi_bc(self, phi, phi_box, geom, mp, moments, stream=None):
        """castro_amd_multipole_phi_bc_fab: the multipole potential on the zones of the one-component FAB `phi` outside the domain"""
        L.check(self.lib.castro_amd_multipole_phi_bc_fab(self.h, C.byref(L.fab_of(phi, *phi_box)), C.byref(geom), C.byref(mp),
                                                         C.c_void_p(moments.data_ptr()), _stream_ptr(stream)), "multipole_phi_bc_fab")

    def poisson_plan_create(self, geom):
        """castro_amd_poisson_plan_create: the multigrid levels of the domain of `geom` and their arrays; a handle for
        poisson_solve / poisson_level_op, freed by poisson_plan_destroy.  ValueError when the coarsest level would hold more
        than _lib.POISSON_MAX_BOTTOM zones."""
        plan = C.c_void_p()
        rc = self.lib.castro_amd_poisson_plan_create(self.h, C.byref(geom), C.byref(plan))
        if rc == L.ERR_UNSUPPORTED:
            n_cell = tuple(geom.domhi[d] - geom.domlo[d] + 1 for d in range(3))
            raise ValueError("poisson_plan_create: n_cell = %s (coarsest multigrid level %s) on a Cartesian domain without periodic "
                             "or Symmetry faces is all this solver takes, with at most %d zones on the coarsest level"
                             % (n_cell, L.poisson_level_extents(n_cell)[-1], L.POISSON_MAX_BOTTOM))
        L.check(rc, "poisson_plan_create")
        return plan

    def poisson_plan_destroy(self, plan):
        if plan is not None and getattr(self, "h", None):
            self.lib.castro_amd_poisson_plan_destroy(self.h, plan)

    def poisson_solve(self, plan, phi, phi_box, rho, rho_box, rho_comp, fourpiG, reltol=1.e-10, abstol=1.e-10, maxiter=40,
                      stream=None):
        """castro_amd_poisson_solve: V-cycles on `phi` (in place) until the residual meets the stopping rule or maxiter cycles.
        Returns (cycles, converged, final_norm, history) -- history: ||b||, max b, the starting norm, then one norm per cycle."""
        cycles, conv, norm = C.c_int(0), C.c_int(0), C.c_double(0.0)
        hist = (C.c_double * (int(maxiter) + 3))()
        L.check(self.lib.castro_amd_poisson_solve(self.h, plan, C.byref(L.fab_of(phi, *phi_box)), C.byref(L.fab_of(rho, *rho_box)),
                                                  int(rho_comp), float(fourpiG), float(reltol), float(abstol), int(maxiter),
                                                  C.byref(cycles), C.byref(conv), C.byref(norm), hist, _stream_ptr(stream)),
                "poisson_solve")
        return cycles.value, bool(conv.value), norm.value, list(hist[:cycles.value + 3])

    def poisson_level_op(self, plan, op, level, a, b=None, c=None, colour=0, out=None, stream=None):
        """castro_amd_poisson_level_op: one pass (_lib.MG_*) on the (tensor, box) pairs a, b, c with the coefficients of `level`"""
        fabs = [C.byref(L.fab_of(*x[:1], *x[1])) if x is not None else None for x in (a, b, c)]
        L.check(self.lib.castro_amd_poisson_level_op(self.h, plan, int(op), int(level), int(colour), fabs[0], fabs[1], fabs[2],
                                                     C.c_void_p(out.data_ptr()) if out is not None else None, _stream_ptr(stream)),
                "poisson_level_op")

    def grad_phi_to_grav(self, phi, phi_box, grav, grav_box, geom, stream=None):
        """castro_amd_grad_phi_to_grav_fab: g = -grad(phi) on the zones of the domain of the 3-component FAB `grav`"""
        L.check(self.lib.castro_amd_grad_phi_to_grav_fab(self.h, C.byref(L.fab_of(phi, *phi_box)), C.byref(L.fab_of(grav, *grav_box)),
                                                         C.byref(geom), _stream_ptr(stream)), "grad_phi_to_grav_fab")

    def poisson_cf_bc(self, phi, phi_box, fine_lo, fine_hi, crse_old, crse_old_box, crse_new, crse_new_box, a, stream=None):
        """castro_amd_poisson_cf_bc_fab: the Dirichlet data of the level solve of the patch [fine_lo, fine_hi] into the one-zone
        shell around it in `phi`, from the potentials of the level below: (1 - a) crse_old + a crse_new, the value on the fine face"""
        rc = self.lib.castro_amd_poisson_cf_bc_fab(self.h, C.byref(L.fab_of(phi, *phi_box)), L.i3(fine_lo), L.i3(fine_hi),
                                                   C.byref(L.fab_of(crse_old, *crse_old_box)), C.byref(L.fab_of(crse_new, *crse_new_box)),
                                                   float(a), _stream_ptr(stream))
        L.check(rc, "poisson_cf_bc_fab")

    # ---- a refined level of several boxes as ONE array over their bounding box BB (k_mgb_* of poisson_kernels.hip).  phi: one
    #      component on BB grown by one; faces: three components on [BB.lo, BB.hi + 1], component d at a zone the value ON its low
    #      d-face ------------------------------------------------------------------------------------------------------------------
    def poisson_boxes_plan_create(self, dx, boxes):
        """castro_amd_poisson_boxes_plan_create: the multigrid levels and coverage flags of the union of `boxes` [(lo, hi)], in
        the zones of the level; freed by poisson_plan_destroy.  Every refusal is a RuntimeError with the error code."""
        n = len(boxes)
        lo = (C.c_int * (3 * max(n, 1)))(*[int(x) for b in boxes for x in b[0]])
        hi = (C.c_int * (3 * max(n, 1)))(*[int(x) for b in boxes for x in b[1]])
        plan = C.c_void_p()
        L.check(self.lib.castro_amd_poisson_boxes_plan_create(self.h, (C.c_double * 3)(*[float(x) for x in dx]), n, lo, hi,
                                                              C.byref(plan)), "poisson_boxes_plan_create")
        return plan

    def poisson_boxes_cf_bc(self, plan, faces, faces_box, crse_old, crse_old_box, crse_new, crse_new_box, a, stream=None):
        """castro_amd_poisson_boxes_cf_bc: the coarse-fine boundary values of the union into the slots of `faces` that lie between
        a covered and an uncovered zone, from the potentials of the level below: (1 - a) crse_old + a crse_new"""
        L.check(self.lib.castro_amd_poisson_boxes_cf_bc(self.h, plan, C.byref(L.fab_of(faces, *faces_box)),
                                                        C.byref(L.fab_of(crse_old, *crse_old_box)),
                                                        C.byref(L.fab_of(crse_new, *crse_new_box)), float(a), _stream_ptr(stream)),
                "poisson_boxes_cf_bc")

    def poisson_boxes_solve(self, plan, phi, phi_box, faces, faces_box, rhos, rho_comp, fourpiG, reltol=1.e-10, abstol=1.e-10,
                            maxiter=40, stream=None):
        """castro_amd_poisson_boxes_solve: poisson_solve on the union; rhos: [(state, box)] of every box of the plan, in its order"""
        cycles, conv, norm = C.c_int(0), C.c_int(0), C.c_double(0.0)
        hist = (C.c_double * (int(maxiter) + 3))()
        L.check(self.lib.castro_amd_poisson_boxes_solve(self.h, plan, C.byref(L.fab_of(phi, *phi_box)), C.byref(L.fab_of(faces, *faces_box)),
                                                        len(rhos), self.make_grav_fabs(rhos), int(rho_comp), float(fourpiG),
                                                        float(reltol), float(abstol), int(maxiter), C.byref(cycles), C.byref(conv),
                                                        C.byref(norm), hist, _stream_ptr(stream)), "poisson_boxes_solve")
        return cycles.value, bool(conv.value), norm.value, list(hist[:cycles.value + 3])

    def grad_phi_to_grav_boxes(self, plan, phi, phi_box, faces, faces_box, gravs, stream=None):
        """castro_amd_grad_phi_to_grav_boxes: g = -grad(phi) on the zones of every box into its own FAB; gravs: [(grav, box)]"""
        L.check(self.lib.castro_amd_grad_phi_to_grav_boxes(self.h, plan, C.byref(L.fab_of(phi, *phi_box)),
                                                           C.byref(L.fab_of(faces, *faces_box)), len(gravs), self.make_grav_fabs(gravs),
                                                           _stream_ptr(stream)), "grad_phi_to_grav_boxes")

    def poisson_boxes_level_op(self, plan, op, level, a, b=None, c=None, faces=None, colour=0, out=None, stream=None):
        """castro_amd_poisson_boxes_level_op: one masked pass (_lib.MG_*) on the (tensor, box) pairs a, b, c over the bounding box
        >> level; faces: the (tensor, box) of the face values (level 0), None: every boundary face holds 0.0"""
        fabs = [C.byref(L.fab_of(*x[:1], *x[1])) if x is not None else None for x in (a, b, c, faces)]
        L.check(self.lib.castro_amd_poisson_boxes_level_op(self.h, plan, int(op), int(level), int(colour), fabs[0], fabs[1], fabs[2],
                                                           fabs[3], C.c_void_p(out.data_ptr()) if out is not None else None,
                                                           _stream_ptr(stream)), "poisson_boxes_level_op")

    # ---- the central point mass (castro.use_point_mass; Gravity.cpp:2903-2948, Castro_pointmass.cpp) ---------------------
    def add_pointmass(self, grav, grav_box, pm, geom, mass, stream=None):
        """castro_amd_add_pointmass_fab: Gravity::add_pointmass_to_gravity over the whole box of the 3-component FAB `grav`; pm:
        _lib.make_pointmass(center, Gconst); mass: a device tensor whose first double is the point mass"""
        L.check(self.lib.castro_amd_add_pointmass_fab(self.h, C.byref(L.fab_of(grav, *grav_box)), C.byref(pm), C.byref(geom),
                                                      C.c_void_p(mass.data_ptr()), _stream_ptr(stream)), "add_pointmass_fab")

    def add_pointmass_mf(self, fabs, pm, geom, mass, stream=None):
        """castro_amd_add_pointmass_mf: add_pointmass for every FAB of `fabs` (make_grav_fabs) in one launch"""
        if len(fabs):
            L.check(self.lib.castro_amd_add_pointmass_mf(self.h, len(fabs), fabs, C.byref(pm), C.byref(geom),
                                                         C.c_void_p(mass.data_ptr()), _stream_ptr(stream)), "add_pointmass_mf")

    @staticmethod
    def make_pointmass_boxes(specs):
        """ctypes array of castro_amd_pointmass_box from (lo, hi, (S_old, box), (S_new, box))."""
        arr = (L.PointMassBox * max(len(specs), 1))()
        for pb, (lo, hi, so, sn) in zip(arr, specs):
            for d in range(3):
                pb.lo[d], pb.hi[d] = lo[d], hi[d]
            pb.state_old, pb.state_new = L.fab_of(so[0], *so[1]), L.fab_of(sn[0], *sn[1])
        return arr, len(specs)

    def pointmass_delta_mf(self, boxes, pm, geom, delta, stream=None):
        """castro_amd_pointmass_delta_mf: the mass that arrived in the 4 x 4 x 4 zones around the centre, over the boxes of `boxes`
        (make_pointmass_boxes), into the first double of the device tensor `delta` (overwritten).  Deterministic."""
        arr, n = boxes
        L.check(self.lib.castro_amd_pointmass_delta_mf(self.h, n, arr, C.byref(pm), C.byref(geom), C.c_void_p(delta.data_ptr()),
                                                       _stream_ptr(stream)), "pointmass_delta_mf")

    def pointmass_apply_mf(self, boxes, pm, geom, delta, mass, stream=None):
        """castro_amd_pointmass_apply_mf: if delta > 0, mass += delta and the cube zones of S_new take S_old's values"""
        arr, n = boxes
        L.check(self.lib.castro_amd_pointmass_apply_mf(self.h, n, arr, C.byref(pm), C.byref(geom), C.c_void_p(delta.data_ptr()),
                                                       C.c_void_p(mass.data_ptr()), _stream_ptr(stream)), "pointmass_apply_mf")

    # ---- tracer particles (castro.do_tracer_particles; castro_amd/particles.py) ------------------------------------------
    @staticmethod
    def make_tracer_boxes(specs):
        """ctypes array of castro_amd_tracer_box from (vlo, vhi, (fab, box) or None): the FAB of a box of a level (None: the
        valid box alone -- for tracer_locate, and in the other tables a box another rank owns, whose particles are not here;
        an int32 tensor: a count FAB) and the valid box inside it."""
        arr = (L.TracerBox * max(len(specs), 1))()
        for i, (vlo, vhi, fab) in enumerate(specs):
            if fab is None:
                arr[i].fab = L.fab_desc(None, vlo, vhi, 0)
            elif fab[0].dtype == torch.int32:
                t, (lo, hi) = fab
                assert t.is_contiguous() and tuple(t.shape[-3:]) == tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0))
                arr[i].fab = L.fab_desc(t.data_ptr(), lo, hi, 1)
            else:
                arr[i].fab = L.fab_of(fab[0], *fab[1])
            arr[i].vlo, arr[i].vhi = L.i3(vlo), L.i3(vhi)
        return arr, len(specs), [s[2][0] for s in specs if s[2] is not None]      # the tensors stay alive with the table

    @staticmethod
    def _tracers(tracers):
        return tracers if isinstance(tracers, L.Tracers) else tracers.struct()

    def tracer_advect(self, level, boxes, geom, dt, ipass, tracers, flags, stream=None, ng=None):
        """castro_amd_tracer_advect_mf: pass `ipass` of AdvectWithUcc over the particles of `level`; boxes: make_tracer_boxes of
        the half-time state; tracers: an _lib.Tracers (or a TracerParticles); flags: two device int32 (clamped, lost).  ng: the
        ghost zones the reference's FillPatch asks for -- not needed here, the stencil is clamped to the whole array"""
        tracers = self._tracers(tracers)
        L.check(self.lib.castro_amd_tracer_advect_mf(self.h, int(level), boxes[1], boxes[0], C.byref(geom), float(dt), int(ipass),
                                                     C.byref(tracers), C.c_void_p(flags.data_ptr()), _stream_ptr(stream)),
                "tracer_advect_mf")

    def tracer_locate(self, lev_min, lev_max, ngrow, level_boxes, geoms, tracers, flags, stream=None):
        """castro_amd_tracer_locate: Redistribute(lev_min, lev_max, ngrow); level_boxes[l]: [(vlo, vhi)] of level l, geoms[l] its
        geometry"""
        nlev, tracers = len(level_boxes), self._tracers(tracers)
        arr, _, _ = self.make_tracer_boxes([(lo, hi, None) for bl in level_boxes for lo, hi in bl])
        cnt = (C.c_int * nlev)(*[len(bl) for bl in level_boxes])
        garr = (L.Geom * nlev)(*geoms)
        L.check(self.lib.castro_amd_tracer_locate(self.h, int(lev_min), int(lev_max), int(ngrow), nlev, cnt, arr, garr,
                                                  C.byref(tracers), C.c_void_p(flags.data_ptr()), _stream_ptr(stream)),
                "tracer_locate")

    def tracer_sample(self, level, boxes, geom, comps, tracers, out, flags, stream=None):
        """castro_amd_tracer_sample_mf: components `comps` of the FABs of `boxes` at the particles of `level` into
        out[c, particle] (a device tensor (len(comps), n))"""
        carr, tracers = (C.c_int * len(comps))(*[int(x) for x in comps]), self._tracers(tracers)
        assert out.is_contiguous() and tuple(out.shape) == (len(comps), int(tracers.n))
        L.check(self.lib.castro_amd_tracer_sample_mf(self.h, int(level), boxes[1], boxes[0], C.byref(geom), len(comps), carr,
                                                     C.byref(tracers), C.c_void_p(out.data_ptr()), C.c_void_p(flags.data_ptr()),
                                                     _stream_ptr(stream)), "tracer_sample_mf")

    def tracer_count(self, level, boxes, geom, tracers, stream=None):
        """castro_amd_tracer_count_mf: += 1 per particle of `level` in its zone of the int32 FABs of `boxes` (make_tracer_boxes)"""
        tracers = self._tracers(tracers)
        L.check(self.lib.castro_amd_tracer_count_mf(self.h, int(level), boxes[1], boxes[0], C.byref(geom), C.byref(tracers),
                                                    _stream_ptr(stream)), "tracer_count_mf")

    def tracer_migrate_count(self, level_owners, nranks, myrank, tracers, dest, counts, stream=None):
        """castro_amd_tracer_migrate_count: level_owners[l]: the owner rank of every box of level l; dest: device int32 (n),
        counts: device int32 (nranks) -- the destination of every particle and the number per destination"""
        nlev, tracers = len(level_owners), self._tracers(tracers)
        flat = [int(o) for ol in level_owners for o in ol]
        cnt = (C.c_int * nlev)(*[len(ol) for ol in level_owners])
        own = (C.c_int * max(len(flat), 1))(*flat)
        assert dest.dtype == torch.int32 and dest.numel() >= int(tracers.n) and counts.dtype == torch.int32 and counts.numel() >= nranks
        L.check(self.lib.castro_amd_tracer_migrate_count(self.h, nlev, cnt, own, int(nranks), int(myrank), C.byref(tracers),
                                                         C.c_void_p(dest.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                         _stream_ptr(stream)), "tracer_migrate_count")

    def tracer_migrate_pack(self, nranks, myrank, tracers, dest, out, wire, stream=None):
        """castro_amd_tracer_migrate_pack after tracer_migrate_count on the same particles: the stayers into `out` (an
        _lib.Tracers of counts[myrank] entries), the leavers into wire, an int64 (nwire, 8) device tensor of 64-byte records"""
        tracers, out = self._tracers(tracers), self._tracers(out)
        assert wire.dtype == torch.int64 and wire.is_contiguous() and wire.dim() == 2 and wire.shape[1] == 8
        L.check(self.lib.castro_amd_tracer_migrate_pack(self.h, int(nranks), int(myrank), C.byref(tracers), C.c_void_p(dest.data_ptr()),
                                                        C.byref(out), C.c_void_p(wire.data_ptr()), int(wire.shape[0]),
                                                        _stream_ptr(stream)), "tracer_migrate_pack")

    def tracer_unpack(self, wire, out, at, stream=None):
        """castro_amd_tracer_unpack: the records of wire (int64 (nrecv, 8)) into out[at, at + nrecv)"""
        out = self._tracers(out)
        assert wire.dtype == torch.int64 and wire.is_contiguous() and wire.dim() == 2 and wire.shape[1] == 8
        L.check(self.lib.castro_amd_tracer_unpack(self.h, C.c_void_p(wire.data_ptr()), int(wire.shape[0]), C.byref(out), int(at),
                                                  _stream_ptr(stream)), "tracer_unpack")

    def sources_mf_g(self, stage, boxes, grav_old, grav_new, grav_source_type, rot, geom, params, dt, ntimes=1, stream=None,
                     sponge=None):
        """castro_amd_sources_mf_g: sources_mf with the gravity of box i read from grav_old[i] / grav_new[i] (make_grav_fabs).
        sponge (_lib.make_sponge with a center): castro_amd_sources_mf_opts, the sponge after rotation in stage 1."""
        arr, n = boxes
        if n and sponge is not None:
            self._sources_mf_opts(stage, arr, n, L.SourceOpts(None, grav_old, grav_new, int(grav_source_type)), rot, None, sponge,
                                  geom, params, dt, ntimes, stream)
            return
        if n:
            L.check(self.lib.castro_amd_sources_mf_g(self.h, int(stage), n, arr, grav_old, grav_new, int(grav_source_type),
                                                     C.byref(rot) if rot is not None else None, C.byref(geom), C.byref(params),
                                                     float(dt), int(ntimes), _stream_ptr(stream)), "sources_mf_g")

    def old_gravity_source_gfab(self, state, box, source, src_box, lo, hi, grav_old, grav_box, grav_source_type, dt, stream=None):
        L.check(self.lib.castro_amd_old_gravity_source_gfab(self.h, C.byref(L.fab_of(state, *box)), C.byref(L.fab_of(source, *src_box)),
                                                            L.i3(lo), L.i3(hi), C.byref(L.fab_of(grav_old, *grav_box)),
                                                            int(grav_source_type), float(dt), _stream_ptr(stream)),
                "old_gravity_source_gfab")

    def new_gravity_source_gfab(self, state_old, old_box, state_new, new_box, source, src_box, mass_fluxes, flux_boxes, lo, hi,
                                grav_old, grav_new, grav_box, grav_source_type, dt, geom, stream=None):
        mb = (L.Fab * 3)()
        for d in range(3):
            mb[d] = L.fab_of(mass_fluxes[d], *flux_boxes[d])
        L.check(self.lib.castro_amd_new_gravity_source_gfab(self.h, C.byref(L.fab_of(state_old, *old_box)),
                                                            C.byref(L.fab_of(state_new, *new_box)),
                                                            C.byref(L.fab_of(source, *src_box)), mb, L.i3(lo), L.i3(hi),
                                                            C.byref(L.fab_of(grav_old, *grav_box)), C.byref(L.fab_of(grav_new, *grav_box)),
                                                            int(grav_source_type), float(dt), C.byref(geom), _stream_ptr(stream)),
                "new_gravity_source_gfab")

    def old_rotation_source(self, state, box, source, src_box, lo, hi, rot, geom, dt, stream=None):
        L.check(self.lib.castro_amd_old_rotation_source_fab(self.h, C.byref(L.fab_of(state, *box)), C.byref(L.fab_of(source, *src_box)),
                                                            L.i3(lo), L.i3(hi), C.byref(rot), C.byref(geom), float(dt),
                                                            _stream_ptr(stream)), "old_rotation_source_fab")

    def new_rotation_source(self, state_old, old_box, state_new, new_box, source, src_box, mass_fluxes, flux_boxes, lo, hi,
                            rot, geom, dt, stream=None):
        mb = (L.Fab * 3)()
        for d in range(3):
            mb[d] = L.fab_of(mass_fluxes[d], *flux_boxes[d])
        L.check(self.lib.castro_amd_new_rotation_source_fab(self.h, C.byref(L.fab_of(state_old, *old_box)),
                                                            C.byref(L.fab_of(state_new, *new_box)),
                                                            C.byref(L.fab_of(source, *src_box)), mb, L.i3(lo), L.i3(hi),
                                                            C.byref(rot), C.byref(geom), float(dt), _stream_ptr(stream)),
                "new_rotation_source_fab")

    def new_sponge_source(self, state_new, new_box, source, src_box, lo, hi, sponge, geom, params, dt, stream=None):
        """castro_amd_new_sponge_source_fab: Castro::construct_new_sponge_source on [lo, hi] (sponge: _lib.make_sponge with a center)"""
        L.check(self.lib.castro_amd_new_sponge_source_fab(self.h, C.byref(L.fab_of(state_new, *new_box)),
                                                          C.byref(L.fab_of(source, *src_box)), L.i3(lo), L.i3(hi), C.byref(sponge),
                                                          C.byref(geom), C.byref(params), float(dt), _stream_ptr(stream)),
                "new_sponge_source_fab")

    def _sources_mf_opts(self, stage, arr, n, opts, rot, diffusion, sponge, geom, params, dt, ntimes, stream):
        """castro_amd_sources_mf_opts with the gravity fields of `opts` set by the caller"""
        if rot is not None:
            opts.rot = C.pointer(rot)
        if diffusion is not None:
            opts.diff = C.pointer(diffusion)
        opts.sponge = C.pointer(sponge)
        L.check(self.lib.castro_amd_sources_mf_opts(self.h, int(stage), n, arr, C.byref(opts), C.byref(geom), C.byref(params),
                                                    float(dt), int(ntimes), _stream_ptr(stream)), "sources_mf_opts")

    def saxpy(self, dst, dst_box, a, src, src_box, ncomp, lo, hi, stream=None):
        """dst[:ncomp] += a * src[:ncomp] on [lo,hi] (Castro::apply_source_to_state)."""
        L.check(self.lib.castro_amd_saxpy_fab(self.h, C.byref(L.fab_of(dst, *dst_box)), float(a), C.byref(L.fab_of(src, *src_box)),
                                              int(ncomp), L.i3(lo), L.i3(hi), _stream_ptr(stream)), "saxpy_fab")

    def apply_source(self, dst, dst_box, base, base_box, a, src, src_box, nsrc, lo, hi, params, ntimes=1, stream=None):
        """dst = base + a * src[:nsrc] (other components copied) followed by clean_state x ntimes, one pass."""
        L.check(self.lib.castro_amd_apply_source_fab(self.h, C.byref(L.fab_of(dst, *dst_box)), C.byref(L.fab_of(base, *base_box)),
                                                     float(a), C.byref(L.fab_of(src, *src_box)), int(nsrc), L.i3(lo), L.i3(hi),
                                                     C.byref(params), int(ntimes), _stream_ptr(stream)), "apply_source_fab")

    # ---- two-level AMR building blocks (include/castro_hydro_amd.h) ------------------------------
    def error_tag(self, field, field_box, comp, tags, tags_box, lo, hi, kind, value, stream=None):
        """kind: 0 value_greater, 1 value_less, 2 gradient, 3 relative_gradient (AMRErrorTag)."""
        L.check(self.lib.castro_amd_error_tag_fab(self.h, C.byref(L.fab_of(field, *field_box)), int(comp),
                                                  C.byref(L.fab_of(tags, *tags_box)), L.i3(lo), L.i3(hi), int(kind),
                                                  float(value), _stream_ptr(stream)), "error_tag_fab")

    def cc_interp(self, crse, crse_box, fine, fine_box, lo, hi, ncomp, stream=None):
        L.check(self.lib.castro_amd_cc_interp_fab(self.h, C.byref(L.fab_of(crse, *crse_box)), C.byref(L.fab_of(fine, *fine_box)),
                                                  L.i3(lo), L.i3(hi), int(ncomp), _stream_ptr(stream)), "cc_interp_fab")

    def fillpatch_shell(self, crse, crse_box, fine, fine_box, vlo, vhi, ngrow, params, ntimes=1, stream=None):
        """cc_interp + clean_state x ntimes on grow([vlo, vhi], ngrow) minus [vlo, vhi], one launch."""
        L.check(self.lib.castro_amd_fillpatch_shell_fab(self.h, C.byref(L.fab_of(crse, *crse_box)), C.byref(L.fab_of(fine, *fine_box)),
                                                        L.i3(vlo), L.i3(vhi), int(ngrow), C.byref(params), int(ntimes),
                                                        _stream_ptr(stream)), "fillpatch_shell_fab")

    @staticmethod
    def make_ops(specs):
        """ctypes array of castro_amd_fab_op from (kind, dir, ncomp, lo, hi, a, b, (dst, box), (src, box), (src2, box) | None);
        for OP_REFLUX `dir` is the pair (dir, side) and `a` the zone volume."""
        arr = (L.FabOp * max(len(specs), 1))()
        for o, (kind, dir_, ncomp, lo, hi, a, b, dst, src, src2) in zip(arr, specs):
            if isinstance(dir_, tuple):
                dir_, o.side = dir_
            o.kind, o.dir, o.ncomp, o.a, o.b = kind, dir_, ncomp, a, b
            for d in range(3):
                o.lo[d], o.hi[d] = lo[d], hi[d]
            o.dst, o.src = L.fab_of(dst[0], *dst[1]), L.fab_of(src[0], *src[1])
            if kind == L.OP_FLUXREG_TO_FLUX:        # src2 is written: the mass-flux FAB, or none
                o.src2 = L.fab_of(src2[0], *src2[1]) if src2 is not None else L.fab_desc(None, lo, hi, 0)
                continue
            o.src2 = L.fab_of(src2[0], *src2[1]) if src2 is not None else o.src
        return arr, len(specs)

    def fab_ops(self, ops, stream=None, params=None):
        """Independent FAB-to-FAB region operations (make_ops): one launch for up to sixteen, and with `params`
        (castro_amd_fab_ops_p: needed by OP_CLEAN / OP_INTERP_CLEAN) one launch for any number.  OP_CLEAN operations run
        clean_state's own kernel, 32 regions per launch, in front of the others."""
        arr, n = ops
        if n:
            if params is not None:
                L.check(self.lib.castro_amd_fab_ops_p(self.h, n, arr, C.byref(params), _stream_ptr(stream)), "fab_ops_p")
            else:
                L.check(self.lib.castro_amd_fab_ops(self.h, n, arr, _stream_ptr(stream)), "fab_ops")

    # ---- checkpoints: the valid zones of many FABs into one buffer and back (castro_amd/checkpoint.py) ----
    @staticmethod
    def make_pack_entries(specs):
        """(ctypes array of castro_amd_pack_entry, n, doubles, pairs) from [(tensor, box, (lo, hi)), ...]: the region [lo, hi] of
        every FAB tensor (ncomp, nz, ny, nx) on `box`, one after the other in the buffer (offsets 0, ncomp x zones, ...); doubles:
        what the regions take together; pairs: the sum of ncomp (the min / max vector has 2 x pairs entries).  The tensors must
        outlive the table."""
        arr = (L.PackEntry * max(len(specs), 1))()
        at, pairs = 0, 0
        for e, (t, box, (lo, hi)) in zip(arr, specs):
            e.fab = L.fab_of(t, *box)
            for d in range(3):
                e.vlo[d], e.vhi[d] = lo[d], hi[d]
            e.offset = at
            at += int(t.shape[0]) * max(hi[0] - lo[0] + 1, 0) * max(hi[1] - lo[1] + 1, 0) * max(hi[2] - lo[2] + 1, 0)
            pairs += int(t.shape[0])
        return arr, len(specs), at, pairs

    def fab_pack(self, entries, dst, minmax=None, stream=None):
        """castro_amd_fab_pack: the regions of `entries` (make_pack_entries) into the 1-D float64 device tensor dst, in the
        on-disk FAB order; minmax: a float64 device tensor of 2 x pairs entries that receives the minimum of every (entry,
        component), then the maxima -- one launch, plus a small one for the reduction."""
        arr, n, doubles, pairs = entries
        if n == 0:
            return
        if dst.dtype != torch.float64 or not dst.is_contiguous() or dst.numel() < doubles:
            raise ValueError("fab_pack: dst must be a contiguous float64 tensor of at least %d entries" % doubles)
        if minmax is not None and (minmax.dtype != torch.float64 or not minmax.is_contiguous() or minmax.numel() < 2 * pairs):
            raise ValueError("fab_pack: minmax must be a contiguous float64 tensor of at least %d entries" % (2 * pairs))
        L.check(self.lib.castro_amd_fab_pack(self.h, n, arr, C.c_void_p(dst.data_ptr()),
                                             C.c_void_p(minmax.data_ptr()) if minmax is not None else None, _stream_ptr(stream)),
                "fab_pack")

    def fab_unpack(self, entries, src, stream=None):
        """castro_amd_fab_unpack: the reverse copy, src into the regions; the zones of the FABs outside them are untouched"""
        arr, n, doubles, _ = entries
        if n == 0:
            return
        if src.dtype != torch.float64 or not src.is_contiguous() or src.numel() < doubles:
            raise ValueError("fab_unpack: src must be a contiguous float64 tensor of at least %d entries" % doubles)
        L.check(self.lib.castro_amd_fab_unpack(self.h, n, arr, C.c_void_p(src.data_ptr()), _stream_ptr(stream)), "fab_unpack")

    @staticmethod
    def make_hydro_boxes(specs):
        """ctypes array of castro_amd_hydro_box from (bx, vbx, (Sborder, box), (S_new, box), fluxes, flux_boxes, mass_fluxes
        [, (src, box)]) -- src: the old-time source FAB of the box (Source_Type data with ghost zones), traced by the call."""
        arr = (L.HydroBox * max(len(specs), 1))()
        for hb, spec in zip(arr, specs):
            bx, vbx, sb, sn, fluxes, flux_boxes, mass_fluxes = spec[:7]
            src = spec[7] if len(spec) > 7 else None
            for d in range(3):
                hb.bxlo[d], hb.bxhi[d], hb.vbxlo[d], hb.vbxhi[d] = bx[0][d], bx[1][d], vbx[0][d], vbx[1][d]
                hb.flux[d] = L.fab_of(fluxes[d], *flux_boxes[d])
                hb.mass_flux[d] = L.fab_of(mass_fluxes[d], *flux_boxes[d])
                hb.qe[d] = L.fab_of(None, *flux_boxes[d])
            hb.Sborder, hb.S_new = L.fab_of(sb[0], *sb[1]), L.fab_of(sn[0], *sn[1])
            hb.src = L.fab_of(src[0], *src[1]) if src is not None else L.fab_desc(None, bx[0], bx[1], 0)
        return arr, len(specs)

    def construct_ctu_hydro_source_mf(self, pool, boxes, geom, params, time, dt, update_from_sborder=True, flux_assign=False,
                                      clean_ntimes=0, red=None, stream=None):
        """castro_amd_ctu_hydro_mf: the hydro update of every box of a level in one call (the MFIter loop).
        pool: [(HipHydro, torch stream)] the boxes are dealt to round robin, or None for this context on the current stream."""
        arr, n = boxes
        if not n:
            return
        flags = L.UPDATE_FROM_SBORDER if update_from_sborder else L.UPDATE_ADD
        if flux_assign:
            flags |= L.FLUX_ASSIGN
        o = L.HydroOpts(flags, int(clean_ntimes), red.data_ptr() if red is not None else None, 0, None)
        main = _stream_ptr(stream)
        if pool:
            ctxs = (C.c_void_p * len(pool))(*[h.h for h, _ in pool])
            sts = (C.c_void_p * len(pool))(*[C.c_void_p(st.cuda_stream) for _, st in pool])
            k = len(pool)
        else:
            ctxs, sts, k = (C.c_void_p * 1)(self.h), (C.c_void_p * 1)(main), 1
        L.check(self.lib.castro_amd_ctu_hydro_mf(ctxs, sts, k, arr, n, C.byref(geom), C.byref(params), float(time), float(dt),
                                                 C.byref(o), main), "ctu_hydro_mf")

    # ---- the per-box stages around the hydro update, for every box of a level in one call ----------------
    @staticmethod
    def make_source_boxes(specs):
        """ctypes array of castro_amd_source_box from (lo, hi, (S_old, box), (S_new, box), (source, box), mass_fluxes, flux_boxes)."""
        arr = (L.SourceBox * max(len(specs), 1))()
        for sb, (lo, hi, so, sn, src, mass_fluxes, flux_boxes) in zip(arr, specs):
            for d in range(3):
                sb.lo[d], sb.hi[d] = lo[d], hi[d]
                sb.mass_flux[d] = L.fab_of(mass_fluxes[d], *flux_boxes[d])
            sb.S_old, sb.S_new, sb.source = L.fab_of(so[0], *so[1]), L.fab_of(sn[0], *sn[1]), L.fab_of(src[0], *src[1])
        return arr, len(specs)

    def sources_mf(self, stage, boxes, grav, grav_source_type, rot, geom, params, dt, ntimes=1, stream=None, diffusion=None,
                   sponge=None):
        """castro_amd_sources_mf: stage 0 = old-time sources + S_new = S_old + dt * source + clean_state, stage 1 = new-time
        sources + S_new += dt * source + clean_state, stage 1 | _lib.SOURCES_AFTER_REFLUX = S_new -= dt * (stored new-time source) + clean_state, then stage 1
        (the re-evaluation after a reflux), for every box of `boxes` (make_source_boxes).  diffusion
        (_lib.make_diffusion): castro_amd_sources_mf_ex, the thermal-diffusion term in front of gravity and rotation.
        sponge (_lib.make_sponge with a center): castro_amd_sources_mf_opts, the sponge after rotation in stage 1."""
        arr, n = boxes
        if n:
            g = (C.c_double * 3)(*[float(x) for x in grav]) if grav is not None else None
            if sponge is not None:
                opts = L.SourceOpts(C.cast(g, C.POINTER(C.c_double)) if g is not None else None, None, None, int(grav_source_type))
                self._sources_mf_opts(stage, arr, n, opts, rot, diffusion, sponge, geom, params, dt, ntimes, stream)
                return
            if diffusion is not None:
                L.check(self.lib.castro_amd_sources_mf_ex(self.h, int(stage), n, arr, g, int(grav_source_type),
                                                          C.byref(rot) if rot is not None else None, C.byref(diffusion),
                                                          C.byref(geom), C.byref(params), float(dt), int(ntimes),
                                                          _stream_ptr(stream)), "sources_mf_ex")
                return
            L.check(self.lib.castro_amd_sources_mf(self.h, int(stage), n, arr, g, int(grav_source_type),
                                                   C.byref(rot) if rot is not None else None, C.byref(geom), C.byref(params),
                                                   float(dt), int(ntimes), _stream_ptr(stream)), "sources_mf")

    # ---- thermal diffusion (Source/diffusion/) -----------------------------------------------------------------
    def temp_diffusion(self, state, box, source, src_box, lo, hi, diffusion, geom, mult=1.0, diff_term=None, diff_term_box=None,
                       stream=None):
        """source(UEDEN, UEINT) += mult * div(k grad T)(state) on [lo, hi] (Castro::add_temp_diffusion_to_source); state holds
        one filled ghost zone around [lo, hi].  diff_term: a one-component FAB for the bare term (source may be None then)."""
        sf = L.fab_of(source, *src_box) if source is not None else L.fab_desc(None, lo, hi, 0)
        df = L.fab_of(diff_term, *diff_term_box) if diff_term is not None else L.fab_desc(None, lo, hi, 0)
        L.check(self.lib.castro_amd_temp_diffusion_fab(self.h, C.byref(L.fab_of(state, *box)), C.byref(sf), C.byref(df), L.i3(lo),
                                                       L.i3(hi), C.byref(diffusion), C.byref(geom), float(mult),
                                                       _stream_ptr(stream)), "temp_diffusion_fab")

    @staticmethod
    def make_diffusion_boxes(specs):
        """ctypes array of castro_amd_diffusion_box from (lo, hi, (state, box), (source, box))."""
        arr = (L.DiffusionBox * max(len(specs), 1))()
        for db, (lo, hi, st, src) in zip(arr, specs):
            for d in range(3):
                db.lo[d], db.hi[d] = lo[d], hi[d]
            db.state, db.source = L.fab_of(st[0], *st[1]), L.fab_of(src[0], *src[1])
        return arr, len(specs)

    def temp_diffusion_mf(self, boxes, diffusion, geom, mult=1.0, stream=None):
        """temp_diffusion for every box of `boxes` (make_diffusion_boxes) in one launch"""
        arr, n = boxes
        if n:
            L.check(self.lib.castro_amd_temp_diffusion_mf(self.h, n, arr, C.byref(diffusion), C.byref(geom), float(mult),
                                                          _stream_ptr(stream)), "temp_diffusion_mf")

    def estdt_temp_diffusion(self, state, box, lo, hi, geom, params, diffusion, max_dt, out, stream=None):
        """Castro::estdt_temp_diffusion: min-reduces 0.5 dx^2 / D over [lo, hi] into `out` (ONE device double the caller
        initialised, e.g. out.fill_(1e200)); the caller multiplies the level minimum by cfl."""
        L.check(self.lib.castro_amd_estdt_temp_diffusion_fab(self.h, C.byref(L.fab_of(state, *box)), L.i3(lo), L.i3(hi),
                                                             C.byref(geom), C.byref(params), C.byref(diffusion), float(max_dt),
                                                             C.c_void_p(out.data_ptr()), _stream_ptr(stream)),
                "estdt_temp_diffusion_fab")

    def estdt_temp_diffusion_mf(self, boxes, geom, params, diffusion, max_dt, out, stream=None):
        arr, n = boxes
        if n:
            L.check(self.lib.castro_amd_estdt_temp_diffusion_mf(self.h, n, arr, C.byref(geom), C.byref(params), C.byref(diffusion),
                                                                float(max_dt), C.c_void_p(out.data_ptr()), _stream_ptr(stream)),
                    "estdt_temp_diffusion_mf")

    @staticmethod
    def make_state_boxes(specs):
        """ctypes array of castro_amd_state_box from (lo, hi, (state, box))."""
        arr = (L.StateBox * max(len(specs), 1))()
        for sb, (lo, hi, st) in zip(arr, specs):
            for d in range(3):
                sb.lo[d], sb.hi[d] = lo[d], hi[d]
            sb.state = L.fab_of(st[0], *st[1])
        return arr, len(specs)

    def clean_state_reduce_mf(self, boxes, geom, params, out, ntimes=1, stream=None):
        arr, n = boxes
        if n:
            L.check(self.lib.castro_amd_clean_state_reduce_mf(self.h, n, arr, C.byref(geom), C.byref(params), int(ntimes),
                                                              C.c_void_p(out.data_ptr()), _stream_ptr(stream)), "clean_state_reduce_mf")

    def estdt_cfl_mf(self, boxes, geom, params, out, stream=None):
        arr, n = boxes
        if n:
            L.check(self.lib.castro_amd_estdt_mf(self.h, n, arr, C.byref(geom), C.byref(params), C.c_void_p(out.data_ptr()),
                                                 _stream_ptr(stream)), "estdt_mf")

    # ---- Castro::sum_integrated_quantities (Source/driver/sum_integrated_quantities.cpp) ---------------------------
    @staticmethod
    def make_diag_boxes(specs):
        """ctypes array of castro_amd_diag_box from (lo, hi, (state, box), mask) -- mask: a uint8 tensor shaped (nz, ny, nx) like
        [lo, hi] on the device of the state (0 = the zone is covered by a finer level), or None.  The array keeps the masks alive."""
        arr = (L.DiagBox * max(len(specs), 1))()
        keep = []
        for db, (lo, hi, st, mask) in zip(arr, specs):
            for d in range(3):
                db.lo[d], db.hi[d] = lo[d], hi[d]
            db.state = L.fab_of(st[0], *st[1])
            if mask is not None:
                shape = (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
                if mask.dtype != torch.uint8 or tuple(mask.shape) != shape or not mask.is_contiguous():
                    raise AssertionError("a diag mask is a contiguous uint8 tensor shaped (nz, ny, nx) of its box: %s %s for %s"
                                         % (mask.dtype, tuple(mask.shape), shape))
                db.mask = mask.data_ptr()
                keep.append(mask)
        arr._masks = keep
        return arr, len(specs)

    def integrated_quantities_mf(self, boxes, geom, center, out, stream=None):
        """castro_amd_integrated_quantities_mf: the 14 sums (_lib.DIAG_*) over the valid zones of every box of `boxes`
        (make_diag_boxes), masked zones skipped, into `out` (a device tensor of _lib.DIAG_N doubles, overwritten; no boxes:
        zeros).  Deterministic: the same boxes give the same bits."""
        arr, n = boxes
        ctr = (C.c_double * 3)(*[float(x) for x in center])
        L.check(self.lib.castro_amd_integrated_quantities_mf(self.h, n, arr, C.byref(geom), C.byref(ctr), C.c_void_p(out.data_ptr()),
                                                             _stream_ptr(stream)), "integrated_quantities_mf")

    def diag_workgroups(self, boxes):
        """workgroups (= rows of partial sums) integrated_quantities_mf launches for `boxes`"""
        arr, n = boxes
        nb = int(self.lib.castro_amd_diag_workgroups(n, arr))
        if nb < 0:
            L.check(nb, "diag_workgroups")
        return nb

    def lincomb(self, dst, dst_box, a, x, x_box, b, y, y_box, ncomp, lo, hi, stream=None):
        L.check(self.lib.castro_amd_lincomb_fab(self.h, C.byref(L.fab_of(dst, *dst_box)), float(a), C.byref(L.fab_of(x, *x_box)),
                                                float(b), C.byref(L.fab_of(y, *y_box)), int(ncomp), L.i3(lo), L.i3(hi),
                                                _stream_ptr(stream)), "lincomb_fab")

    def avgdown(self, fine, fine_box, crse, crse_box, lo, hi, ncomp, stream=None):
        L.check(self.lib.castro_amd_avgdown_fab(self.h, C.byref(L.fab_of(fine, *fine_box)), C.byref(L.fab_of(crse, *crse_box)),
                                                L.i3(lo), L.i3(hi), int(ncomp), _stream_ptr(stream)), "avgdown_fab")

    def fluxreg_crse_init(self, reg, reg_box, cflux, cflux_box, lo, hi, ncomp, mult, stream=None):
        L.check(self.lib.castro_amd_fluxreg_crse_init_fab(self.h, C.byref(L.fab_of(reg, *reg_box)), C.byref(L.fab_of(cflux, *cflux_box)),
                                                          L.i3(lo), L.i3(hi), int(ncomp), float(mult), _stream_ptr(stream)),
                "fluxreg_crse_init_fab")

    def fluxreg_fine_add(self, reg, reg_box, fflux, fflux_box, lo, hi, dir, ncomp, mult, stream=None):
        L.check(self.lib.castro_amd_fluxreg_fine_add_fab(self.h, C.byref(L.fab_of(reg, *reg_box)), C.byref(L.fab_of(fflux, *fflux_box)),
                                                         L.i3(lo), L.i3(hi), int(dir), int(ncomp), float(mult), _stream_ptr(stream)),
                "fluxreg_fine_add_fab")

    def reflux(self, state, state_box, reg, reg_box, lo, hi, dir, side, ncomp, vol, stream=None):
        L.check(self.lib.castro_amd_reflux_fab(self.h, C.byref(L.fab_of(state, *state_box)), C.byref(L.fab_of(reg, *reg_box)),
                                               L.i3(lo), L.i3(hi), int(dir), int(side), int(ncomp), float(vol), _stream_ptr(stream)),
                "reflux_fab")

    def fluxreg_to_flux(self, flux, flux_box, reg, reg_box, mass_flux, mass_box, lo, hi, ncomp, stream=None):
        """castro_amd_fluxreg_to_flux_fab: flux += reg on the faces [lo, hi]; mass_flux (or None) = component URHO of the sum"""
        mf = C.byref(L.fab_of(mass_flux, *mass_box)) if mass_flux is not None else None
        L.check(self.lib.castro_amd_fluxreg_to_flux_fab(self.h, C.byref(L.fab_of(flux, *flux_box)), C.byref(L.fab_of(reg, *reg_box)),
                                                        mf, L.i3(lo), L.i3(hi), int(ncomp), _stream_ptr(stream)),
                "fluxreg_to_flux_fab")

    # ---- derived plotfile fields (Source/driver/Derive.cpp) ---------------------------------
    def derive(self, name, state, box, der, der_box, dcomp, lo, hi, geom, params, center, stream=None):
        ctr = (C.c_double * 3)(*[float(x) for x in center])
        L.check(self.lib.castro_amd_derive_fab(self.h, L.DERIVE_IDS[name], C.byref(L.fab_of(state, *box)),
                                               C.byref(L.fab_of(der, *der_box)), int(dcomp), L.i3(lo), L.i3(hi),
                                               C.byref(geom), C.byref(params), C.byref(ctr), _stream_ptr(stream)),
                "derive_fab")

    def step_control(self, red, ctl, params, max_dt=1.e200, fixed_dt=-1.0, stop_time=-1.0, use_retry=False, stream=None):
        """castro_amd_step_control: do_advance_ctu's checks, time += dt and computeNewDt on the device (one thread)."""
        L.check(self.lib.castro_amd_step_control(self.h, C.c_void_p(red.data_ptr()), C.c_void_p(ctl.data_ptr()), C.byref(params),
                                                 float(max_dt), float(fixed_dt), float(stop_time), 1 if use_retry else 0,
                                                 _stream_ptr(stream)),
                "step_control")

    # ---- Castro::clean_state ---------------------------------------------------------------
    def clean_state(self, state, box, lo, hi, params, ntimes=1, stream=None):
        L.check(self.lib.castro_amd_clean_state_fab(self.h, C.byref(L.fab_of(state, *box)), L.i3(lo), L.i3(hi),
                                                    C.byref(params), int(ntimes), _stream_ptr(stream)), "clean_state_fab")

    def clean_state_reduce(self, state, box, lo, hi, geom, params, out, ntimes=1, stream=None):
        """min-density check + clean_state + estdt in one pass (see castro_amd_clean_state_reduce_fab)."""
        L.check(self.lib.castro_amd_clean_state_reduce_fab(self.h, C.byref(L.fab_of(state, *box)), L.i3(lo), L.i3(hi),
                                                           C.byref(geom), C.byref(params), int(ntimes),
                                                           C.c_void_p(out.data_ptr()), _stream_ptr(stream)),
                "clean_state_reduce_fab")

    # ---- Castro::estdt_cfl + S_new.min(URHO) -------------------------------------------------
    def estdt_cfl(self, state, box, lo, hi, geom, params, out, stream=None):
        """Reduces into `out` (device tensor of 2 doubles: [min dx/(c+|u|), min rho]); the caller
        initialises it (e.g. out.fill_(1e200))."""
        L.check(self.lib.castro_amd_estdt_fab(self.h, C.byref(L.fab_of(state, *box)), L.i3(lo), L.i3(hi),
                                              C.byref(geom), C.byref(params), C.c_void_p(out.data_ptr()),
                                              _stream_ptr(stream)), "estdt_fab")

    # ---- FillPatch pieces --------------------------------------------------------------------
    def bc_fill(self, state, box, geom, stream=None):
        L.check(self.lib.castro_amd_bc_fill_fab(self.h, C.byref(L.fab_of(state, *box)), C.byref(geom),
                                                _stream_ptr(stream)), "bc_fill_fab")

    def ext_bc_fill(self, state, box, geom, params, ext, unconverged=None, stream=None):
        """castro_amd_ext_bc_fill_fab: the ambient fill and the hydrostatic fill of the zones of `state` outside the domain, after
        the generic fill (bc_fill, or a fill_boundary with a geometry).  unconverged: an int32 tensor of one element on the
        device to which every column that leaves its Newton loop unconverged adds 1"""
        if unconverged is not None and (unconverged.dtype != torch.int32 or unconverged.numel() != 1 or not unconverged.is_cuda):
            raise ValueError("ext_bc_fill: unconverged must be one int32 on the device")
        rc = self.lib.castro_amd_ext_bc_fill_fab(self.h, C.byref(L.fab_of(state, *box)), C.byref(geom), C.byref(params), C.byref(ext),
                                                 None if unconverged is None else unconverged.data_ptr(), _stream_ptr(stream))
        if rc in (-1, -2):                # CASTRO_AMD_ERR_ARG, CASTRO_AMD_ERR_UNSUPPORTED
            L.check_ext_bc(ext, geom)
        L.check(rc, "ext_bc_fill_fab")

    def copy(self, dst, dst_box, src, src_box, lo, hi, stream=None):
        L.check(self.lib.castro_amd_copy_fab(self.h, C.byref(L.fab_of(dst, *dst_box)), C.byref(L.fab_of(src, *src_box)),
                                             L.i3(lo), L.i3(hi), _stream_ptr(stream)), "copy_fab")

    def pack(self, state, box, lo, hi, buf, stream=None):
        L.check(self.lib.castro_amd_pack_fab(self.h, C.byref(L.fab_of(state, *box)), L.i3(lo), L.i3(hi),
                                             C.c_void_p(buf.data_ptr()), _stream_ptr(stream)), "pack_fab")

    def unpack(self, state, box, lo, hi, buf, stream=None):
        L.check(self.lib.castro_amd_unpack_fab(self.h, C.byref(L.fab_of(state, *box)), L.i3(lo), L.i3(hi),
                                               C.c_void_p(buf.data_ptr()), _stream_ptr(stream)), "unpack_fab")

    # ---- problem setups ----------------------------------------------------------------------
    @staticmethod
    def region_table(boxes, offsets):
        """ctypes arrays for pack_regions / unpack_regions: boxes [(lo, hi)], offsets in doubles."""
        n = len(boxes)
        lo = (C.c_int * (3 * n))(*[x for b in boxes for x in b[0]])
        hi = (C.c_int * (3 * n))(*[x for b in boxes for x in b[1]])
        off = (C.c_longlong * n)(*offsets)
        return n, lo, hi, off

    def pack_regions(self, state, box, table, buf, stream=None):
        """Every region of `table` (region_table) of the FAB into its slice of `buf`, one launch."""
        n, lo, hi, off = table
        L.check(self.lib.castro_amd_pack_regions_fab(self.h, C.byref(L.fab_of(state, *box)), n, lo, hi, off,
                                                     C.c_void_p(buf.data_ptr()), _stream_ptr(stream)), "pack_regions_fab")

    def unpack_regions(self, state, box, table, buf, stream=None):
        n, lo, hi, off = table
        L.check(self.lib.castro_amd_unpack_regions_fab(self.h, C.byref(L.fab_of(state, *box)), n, lo, hi, off,
                                                       C.c_void_p(buf.data_ptr()), _stream_ptr(stream)), "unpack_regions_fab")

    # ---- FillBoundary on RCCL behind the C ABI (castro_amd/csrc/halo_rccl.hip) -----------------------------------
    def comm_version(self):
        return self.lib.castro_amd_comm_version().decode()

    def comm_unique_id(self):
        """ncclGetUniqueId: 128 bytes for the host to hand to every rank"""
        buf = C.create_string_buffer(128)
        L.check(self.lib.castro_amd_comm_unique_id(buf), "comm_unique_id")
        return bytes(buf.raw)

    def comm_create(self, nranks, rank, unique_id):
        """ncclCommInitRank (collective over the ranks): an opaque castro_amd_comm handle"""
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        L.check(self.lib.castro_amd_comm_create(C.byref(h), int(nranks), int(rank), buf, int(self.device.index or 0)), "comm_create")
        return h

    def comm_destroy(self, comm):
        if comm:
            self.lib.castro_amd_comm_destroy(comm)

    def halo_plan(self, comm, regions, ncomp):
        """regions: [(peer, sbox (lo, hi), rbox (lo, hi), send_tag, recv_tag)] -> castro_amd_halo_plan handle"""
        n = len(regions)
        arr = (L.HaloRegion * max(n, 1))()
        for r, (peer, sbox, rbox, stag, rtag) in zip(arr, regions):
            r.peer, r.send_tag, r.recv_tag = int(peer), int(stag), int(rtag)
            for d in range(3):
                r.sbox_lo[d], r.sbox_hi[d] = int(sbox[0][d]), int(sbox[1][d])
                r.rbox_lo[d], r.rbox_hi[d] = int(rbox[0][d]), int(rbox[1][d])
        h = C.c_void_p()
        L.check(self.lib.castro_amd_halo_plan_create(C.byref(h), comm, n, arr, int(ncomp)), "halo_plan_create")
        return h

    def halo_plan_destroy(self, plan):
        if plan:
            self.lib.castro_amd_halo_plan_destroy(plan)

    def halo_plan_bytes_sent(self, plan):
        return int(self.lib.castro_amd_halo_plan_bytes_sent(plan))

    def fill_boundary(self, plan, state, box, geom=None, stream=None):
        """pack -> grouped ncclSend / ncclRecv -> unpack -> physical BC fill, enqueued on the stream"""
        L.check(self.lib.castro_amd_fill_boundary(self.h, plan, C.byref(L.fab_of(state, *box)),
                                                  C.byref(geom) if geom is not None else None, _stream_ptr(stream)), "fill_boundary")

    def fill_boundary_ex(self, plan, state, box, geom=None, stream=None):
        """fill_boundary + the plan's "packed" event recorded behind the pack launch (the last read of the valid zones)"""
        L.check(self.lib.castro_amd_fill_boundary_ex(self.h, plan, C.byref(L.fab_of(state, *box)),
                                                     C.byref(geom) if geom is not None else None, 0, _stream_ptr(stream)), "fill_boundary_ex")

    def halo_plan_wait_packed(self, plan, stream=None):
        """`stream` (default: the current one) waits until the last fill_boundary_ex of `plan` has packed"""
        L.check(self.lib.castro_amd_halo_plan_wait_packed(plan, _stream_ptr(stream)), "halo_plan_wait_packed")

    # ---- several boxes per rank: one grouped exchange for all local FABs of a level (castro_amd_halo_group_*) ----------------
    def halo_group(self, comm, nfabs, sends, recvs, ncomp):
        """sends / recvs: [(fab, peer, (lo, hi), tag)] as castro_amd.halo.level_messages derives them -> castro_amd_halo_group handle"""
        def arr(msgs):
            a = (L.HaloMsg * max(len(msgs), 1))()
            for m, (fab, peer, box, tag) in zip(a, msgs):
                m.fab, m.peer, m.tag = int(fab), int(peer), int(tag)
                for d in range(3):
                    m.lo[d], m.hi[d] = int(box[0][d]), int(box[1][d])
            return a
        h = C.c_void_p()
        L.check(self.lib.castro_amd_halo_group_create(C.byref(h), comm, int(nfabs), len(sends), arr(sends), len(recvs), arr(recvs), int(ncomp)),
                "halo_group_create")
        return h

    def halo_group_destroy(self, group):
        if group:
            self.lib.castro_amd_halo_group_destroy(group)

    def halo_group_bytes_sent(self, group):
        return int(self.lib.castro_amd_halo_group_bytes_sent(group))

    def fill_boundary_group(self, group, states, boxes, geom=None, stream=None):
        """states[f], boxes[f]: tensor and index box of local FAB f"""
        fabs = (L.Fab * len(states))(*[L.fab_of(t, *b) for t, b in zip(states, boxes)])
        L.check(self.lib.castro_amd_fill_boundary_group(self.h, group, fabs, C.byref(geom) if geom is not None else None,
                                                        _stream_ptr(stream)), "fill_boundary_group")

    def fill_boundary_group_ex(self, group, states, boxes, geom=None, stream=None):
        """fill_boundary_group + the group's "packed" event recorded behind the last pack launch"""
        fabs = (L.Fab * len(states))(*[L.fab_of(t, *b) for t, b in zip(states, boxes)])
        L.check(self.lib.castro_amd_fill_boundary_group_ex(self.h, group, fabs, C.byref(geom) if geom is not None else None, 0,
                                                           _stream_ptr(stream)), "fill_boundary_group_ex")

    def halo_group_wait_packed(self, group, stream=None):
        L.check(self.lib.castro_amd_halo_group_wait_packed(group, _stream_ptr(stream)), "halo_group_wait_packed")

    def allreduce_min_c(self, comm, t, stream=None):
        L.check(self.lib.castro_amd_allreduce_min(comm, C.c_void_p(t.data_ptr()), int(t.numel()), _stream_ptr(stream)), "allreduce_min")

    def sedov_init(self, state, box, lo, hi, geom, params, r_init=0.01, p_ambient=1.e-5, exp_energy=1.0,
                   dens_ambient=1.0, nsub=10, stream=None):
        L.check(self.lib.castro_amd_sedov_init_fab(self.h, C.byref(L.fab_of(state, *box)), L.i3(lo), L.i3(hi),
                                                   C.byref(geom), C.byref(params), r_init, p_ambient, exp_energy,
                                                   dens_ambient, int(nsub), _stream_ptr(stream)), "sedov_init_fab")

    def sod_init(self, state, box, lo, hi, geom, params, rho_l, u_l, p_l, rho_r, u_r, p_r, idir=1, frac=0.5,
                 stream=None):
        L.check(self.lib.castro_amd_sod_init_fab(self.h, C.byref(L.fab_of(state, *box)), L.i3(lo), L.i3(hi),
                                                 C.byref(geom), C.byref(params), rho_l, u_l, p_l, rho_r, u_r, p_r,
                                                 int(idir), float(frac), _stream_ptr(stream)), "sod_init_fab")

    # ---- profiling ---------------------------------------------------------------------------
    def profile(self, enable=True):
        self.lib.castro_amd_ctx_profile(self.h, 1 if enable else 0)

    def profile_reset(self):
        self.lib.castro_amd_ctx_profile_reset(self.h)

    def profile_report(self):
        """{kernel name: (total_ms, launches)} measured with hipEvents on the launch stream."""
        out = {}
        n = self.lib.castro_amd_ctx_profile_count(self.h)
        for i in range(n):
            name = C.create_string_buffer(64)
            ms = C.c_double()
            cnt = C.c_longlong()
            self.lib.castro_amd_ctx_profile_get(self.h, i, name, 64, C.byref(ms), C.byref(cnt))
            out[name.value.decode()] = (ms.value, cnt.value)
        return out

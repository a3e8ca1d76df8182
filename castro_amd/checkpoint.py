"""Checkpoint and restart (amr.check_int / amr.check_file / amr.restart) for Castro and CastroAmr.

Reference behaviour restated:
  Castro::checkPoint / Castro::restart     Source/driver/Castro_io.cpp:67-365, 376-473: the files Castro owns -- CastroHeader
                                           ("Checkpoint version: 10"), state_names.txt, point_mass, CPUtime, job_info
  Amr::checkPoint, AmrLevel::checkPoint,   [3P, AMReX; not in the reference tree]: the text `Header` and one VisMF MultiFab per
  StateData::checkPoint                    level and state type.  The layout is restated from their published description and
                                           is UNPINNED: it cannot be checked against an AMReX reader here, and a
                                           checkpoint written by the reference itself is not read.

A checkpoint is the directory <check_file>NNNNN (the coarse step number).  It is written as <name>.temp and renamed once every
rank has finished, so a reader never sees half of one.

  CastroHeader, state_names.txt, point_mass, CPUtime, job_info      as above; point_mass only with castro.use_point_mass
  Header                                   version line, space dimension, cumulative time, max_level, finest_level, the geometry
                                           of every level, refinement ratios, dt_level, dt_min, n_cycle, level_steps, level_count,
                                           then per existing level its number, its box array and per state type `k ncomp`, the
                                           domain box, the new-time interval (two lines), `1` and the MultiFab path
  Level_l/SD_<k>_New_MF_H, .._D_nnnnn      the VisMF files of castro_amd/plotfile.py (one data file per rank, its FABs one after
                                           the other, nGrow 0); k is the index in the reference's enum StateType of a build with
                                           gravity: 0 = State_Type (8 components), 3 = Source_Type (7, with source terms only).
                                           New data only (castro.dump_old = 0).
  castro_amd_state.json                    ours: the driver state AMReX has no slot for (dt, lastDt, the carried CFL estimate,
                                           nsubcycles, per level lastDt and the cached estimate, the rank grid, ...); doubles as
                                           float.hex() strings
  Particles/Header, Particles/DATA_nnnnn   ours, with tracer particles: per rank the arrays pos (3, n) and r (3, n) float64,
                                           ints (4, n) int32 and the two flag words, raw little-endian; the header lists the counts

What a checkpoint holds is what the next coarse step reads and does not compute again from S_new: the valid zones of S_new of
every box, with source terms the new-time source (create_source_corrector and the predictor read it), time / nstep / dt / lastDt,
the CFL estimate the last step carried out of its fused reduction (it may be None), nsubcycles, dt_level and level_count, the
point mass, the particle arrays.  Ghost zones, grav_old / grav_new, the flux registers and the fluxes are made again by the next
step.  Ids of tracer particles are handed out once, by init_particles: there is no counter to save.

On the device the valid zones are packed into one staging buffer by ONE launch per level (HipHydro.fab_pack:
castro_amd_fab_pack), which also reduces the minimum and maximum of every FAB and component that the VisMF headers list; a
backend without the operation (the CPU backend of the tests) is sliced box by box with torch.  With background=True the staging
buffer is copied to pinned host memory on a side stream behind an event and ONE Python thread writes the files once the event
has fired; the steps go on meanwhile.  The thread issues no collective: on more than one rank the gather of the box headers, the
barrier and the rename happen in the next collective call of the driver (the next checkpoint, checkpoint_wait() or close()).
"""
import json
import os
import re
import shutil
import threading
import time as _time

import numpy as np
import torch

from . import _lib as L
from . import plotfile as PF

CASTRO_VERSION = 10                     # Castro_io.cpp: current_version
HEADER_VERSION = "CheckPointVersion_1.0"
STATE_TYPE, SOURCE_TYPE = 0, 3          # enum StateType (Castro.H) with GRAVITY: State, PhiGrav, Gravity, Source
NSRC = 7
STATE_FILE = "castro_amd_state.json"


def _g(x):
    return "%.17g" % x


def _hex(x):
    return None if x is None else float(x).hex()


def _unhex(s):
    return None if s is None else float.fromhex(s)


def _is_amr(run):
    return hasattr(run, "lev")


def _comm(run):
    return run.comm


def _hydro(run):
    return run._hydro_for(0) if _is_amr(run) else run.hydro


def _levels(run):
    """[dict(geom, boxes=[(lo, hi)], mine=[(index in boxes, box object)])], coarsest first"""
    if _is_amr(run):
        return [dict(geom=lev.geom, boxes=[(tuple(b.lo), tuple(b.hi)) for b in lev.boxes],
                     mine=[(i, b) for i, b in enumerate(lev.boxes) if b.owned]) for lev in run.lev]
    return [dict(geom=run.geom, boxes=[(tuple(lo), tuple(hi)) for lo, hi in run._rank_boxes()], mine=[(run.comm.rank, run)])]


def _have_sources(run):
    return bool(run.lev[0].have_sources if _is_amr(run) else run.have_sources)


def _state_types(run):
    return [(STATE_TYPE, L.NUM_STATE)] + ([(SOURCE_TYPE, NSRC)] if _have_sources(run) else [])


def _fab_of(b, k):
    """(tensor, its box) of state type k of box object b"""
    return (b.S_new_b, b.gbox) if k == STATE_TYPE else (b.new_source, b.bx)


def _nzones(lo, hi):
    return (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1)


def _valid(t, box, lo, hi):
    """the view of region [lo, hi] of a FAB tensor (ncomp, nz, ny, nx) on `box`"""
    o = box[0]
    return t[:, lo[2] - o[2]:hi[2] - o[2] + 1, lo[1] - o[1]:hi[1] - o[1] + 1, lo[0] - o[0]:hi[0] - o[0] + 1]


# ---- pack / unpack: the backend's one launch, or torch box by box ------------------------------------------------------------
def pack(hydro, specs, dst, minmax=None):
    """specs = [(tensor, box, (lo, hi))]: the valid regions, in the on-disk FAB order, one after the other into dst; minmax
    (2 x sum(ncomp)): the minima of every (entry, component), then the maxima.  A NaN in a region propagates into both, in
    the kernel as in torch's amin / amax here and numpy's in the plotfile writer."""
    if not specs:
        return
    if hasattr(hydro, "fab_pack"):
        hydro.fab_pack(hydro.make_pack_entries(specs), dst, minmax)
        return
    at, m, M = 0, 0, sum(int(t.shape[0]) for t, _, _ in specs)
    for t, box, (lo, hi) in specs:
        v = _valid(t, box, lo, hi)
        n = v.numel()
        dst[at:at + n] = v.reshape(-1)
        if minmax is not None:
            nc = int(t.shape[0])
            flat = v.reshape(nc, -1)
            minmax[m:m + nc] = flat.amin(dim=1)
            minmax[M + m:M + m + nc] = flat.amax(dim=1)
            m += nc
        at += n


def unpack(hydro, specs, src):
    """the reverse copy: the valid regions only, the ghost zones of the destinations untouched"""
    if not specs:
        return
    if hasattr(hydro, "fab_unpack"):
        hydro.fab_unpack(hydro.make_pack_entries(specs), src)
        return
    at = 0
    for t, box, (lo, hi) in specs:
        v = _valid(t, box, lo, hi)
        n = v.numel()
        v.copy_(src[at:at + n].reshape(v.shape))
        at += n


# ---- one checkpoint in flight ---------------------------------------------------------------------------------------------------
class _Job:
    """A checkpoint from the snapshot to the rename.  snapshot() runs on the stepping stream; write_local() touches host memory
    and this rank's files only (the background thread); finalize() is collective."""

    def __init__(self, run, dirname):
        self.dirname = dirname.rstrip("/")
        self.temp = self.dirname + ".temp"
        self.comm = _comm(run)
        self.rank, self.size = self.comm.rank, self.comm.size
        self.thread, self.error, self.local, self.finalized = None, None, None, False
        self.event, self._keep = None, None
        self._snapshot(run)

    # -- on the stepping stream --------------------------------------------------------------------------------------------------
    def _snapshot(self, run):
        hydro = _hydro(run)
        levels = _levels(run)
        types = _state_types(run)
        self.types = types
        # this rank's FABs in file order: level, state type, box
        self.fabs, per_level, T, M = [], [], 0, 0
        for l, lev in enumerate(levels):
            specs = []
            for k, nc in types:
                for i, b in lev["mine"]:
                    t, box = _fab_of(b, k)
                    specs.append((t, box, (tuple(b.lo), tuple(b.hi))))
                    self.fabs.append(dict(level=l, k=k, index=i, lo=tuple(b.lo), hi=tuple(b.hi), ncomp=nc, at=T))
                    T += nc * _nzones(b.lo, b.hi)
            per_level.append(specs)
            M += sum(int(t.shape[0]) for t, _, _ in specs)
        self.T, self.M = T, M
        pm = getattr(run, "pm", None)
        need = T + 2 * M + 1
        dev = hydro.device
        stage = run.__dict__.get("_ckpt_stage")
        if stage is None or stage.numel() < need or stage.device != dev:
            # allocated on first use, sized to the valid data, kept (a regrid that grows the hierarchy allocates again)
            stage = run._ckpt_stage = torch.empty(need, dtype=torch.float64, device=dev)
            run._ckpt_host = torch.empty(need, dtype=torch.float64, pin_memory=True) if dev.type == "cuda" else None
        at, m = 0, 0
        self.mm_at = []                         # per level: where its minima start in the minmax part, and its count
        for specs in per_level:
            n = sum(int(t.shape[0]) * _nzones(lo, hi) for t, _, (lo, hi) in specs)
            Ml = sum(int(t.shape[0]) for t, _, _ in specs)
            pack(hydro, specs, stage[at:at + n], stage[T + 2 * m:T + 2 * m + 2 * Ml])
            self.mm_at.append((2 * m, Ml))
            at += n
            m += Ml
        if pm is not None:
            stage[T + 2 * M:T + 2 * M + 1].copy_(pm.buf[:1])        # the device double, read with everything else
        tr = getattr(run, "tracers", None)
        self.have_tracers = tr is not None
        if tr is not None and tr.pos is None:
            raise RuntimeError("writeCheckpoint: the tracer particles have not been initialised")
        # The particle arrays are written in place by the steps that follow (advect, locate, the flag reset): like the state
        # and the point mass they are snapshotted ON THE STEPPING STREAM, and the side stream copies the snapshot only
        snaps = [p.clone() for p in (tr.pos, tr.r, tr.ints, tr.flags)] if tr is not None else []
        if dev.type == "cuda":
            host = run._ckpt_host
            side = run.__dict__.get("_ckpt_stream")
            if side is None:
                side = run._ckpt_stream = torch.cuda.Stream(device=dev)
            packed = torch.cuda.Event()
            packed.record()                     # behind the pack, the point-mass copy and the particle snapshots
            side.wait_event(packed)
            with torch.cuda.stream(side):
                host[:need].copy_(stage[:need], non_blocking=True)
                self.parts = []
                for p in snaps:
                    hp = torch.empty(p.shape, dtype=p.dtype, pin_memory=True)
                    hp.copy_(p, non_blocking=True)
                    self.parts.append(hp)
                self.event = torch.cuda.Event()
                self.event.record(side)
            self.host = host
            # what the side stream reads stays alive with the job, whatever becomes of the run object, until the event has fired
            self._keep = (stage, snaps)
        else:
            self.host = stage                   # host memory already, and a copy: the steps that follow do not touch it
            self.parts = snaps
        self.meta = _driver_state(run)
        self.use_point_mass = pm is not None
        self.header = _header_text(run, levels, types)
        self.job_info = _job_info(run)
        self.box_counts = [len(lev["boxes"]) for lev in levels]
        # CPUtime: the wall time of the run so far, over its restarts (counted from the object's first checkpoint call or restart)
        start = run.__dict__.setdefault("_wall_start", _time.perf_counter())
        self.cpu_time = run.__dict__.get("_cpu_time_base", 0.0) + max(_time.perf_counter() - start, 0.0)

    # -- host memory and this rank's files only --------------------------------------------------------------------------------
    def write_local(self):
        if self.event is not None:
            self.event.synchronize()            # the one device call of the background thread
            self._keep = None
        buf = self.host.numpy()
        nlev = len(self.box_counts)
        for l in range(nlev):
            os.makedirs(os.path.join(self.temp, "Level_%d" % l), exist_ok=True)
        local = []
        m = {l: 0 for l in range(nlev)}
        for l in range(nlev):
            for k, nc in self.types:
                mine = [f for f in self.fabs if f["level"] == l and f["k"] == k]
                fname = "SD_%d_New_MF_D_%05d" % (k, self.rank)
                arrs = []
                for f in mine:
                    n = [f["hi"][d] - f["lo"][d] + 1 for d in range(3)]
                    arrs.append((f["lo"], f["hi"], buf[f["at"]:f["at"] + nc * n[0] * n[1] * n[2]].reshape(nc, n[2], n[1], n[0])))
                if not mine:
                    continue
                offs = PF.write_fab_file(os.path.join(self.temp, "Level_%d" % l, fname), arrs)
                mm0, Ml = self.mm_at[l]
                for f, off in zip(mine, offs):
                    a = self.T + mm0 + m[l]
                    local.append(dict(level=l, k=k, index=f["index"], lo=f["lo"], hi=f["hi"], file=fname, offset=off,
                                      min=[float(x) for x in buf[a:a + nc]], max=[float(x) for x in buf[a + Ml:a + Ml + nc]]))
                    m[l] += nc
        count = None
        if self.have_tracers:
            os.makedirs(os.path.join(self.temp, "Particles"), exist_ok=True)
            with open(os.path.join(self.temp, "Particles", "DATA_%05d" % self.rank), "wb") as f:
                for p in self.parts:
                    f.write(np.ascontiguousarray(p.numpy()).tobytes())
            count = int(self.parts[0].shape[1])
        self.point_mass = float(buf[self.T + 2 * self.M]) if self.use_point_mass else None
        self.local = dict(fabs=local, particles=count)

    # -- collective ---------------------------------------------------------------------------------------------------------------
    def finalize(self):
        """the box headers of all ranks to the I/O rank, its text files, the barrier and the rename; every rank raises if one
        rank's write failed"""
        if self.finalized:
            return
        self.finalized = True
        err = None if self.error is None else "%s: %s" % (type(self.error).__name__, self.error)
        parts = self.comm.gather_objects((err, self.local))
        bad = [(r, e) for r, (e, _) in enumerate(parts) if e is not None]
        if bad:
            if self.error is not None:
                raise self.error
            raise RuntimeError("writeCheckpoint %s: rank %d failed: %s" % (self.dirname, bad[0][0], bad[0][1]))
        if self.rank == 0:
            self._write_text([p for _, p in parts])
        self.comm.barrier()
        if self.rank == 0:
            if os.path.isdir(self.dirname):
                shutil.rmtree(self.dirname)
            os.rename(self.temp, self.dirname)
        self.comm.barrier()

    def _write_text(self, parts):
        t = self.temp
        for l, nb in enumerate(self.box_counts):
            for k, nc in self.types:
                fabs = sorted([f for p in parts for f in p["fabs"] if f["level"] == l and f["k"] == k], key=lambda f: f["index"])
                assert len(fabs) == nb, "level %d: %d of %d boxes were written" % (l, len(fabs), nb)
                PF.write_vismf_header(os.path.join(t, "Level_%d" % l, "SD_%d_New_MF_H" % k), nc, fabs)
        with open(os.path.join(t, "Header"), "w") as f:
            f.write(self.header)
        with open(os.path.join(t, "CastroHeader"), "w") as f:
            f.write("Checkpoint version: %d\n" % CASTRO_VERSION)
        with open(os.path.join(t, "state_names.txt"), "w") as f:
            f.write("".join(nm + "\n" for nm in PF.STATE_NAMES))
        with open(os.path.join(t, "CPUtime"), "w") as f:
            f.write(_g(self.cpu_time))
        with open(os.path.join(t, "job_info"), "w") as f:
            f.write(self.job_info)
        if self.use_point_mass:
            with open(os.path.join(t, "point_mass"), "w") as f:
                f.write(_g(self.point_mass) + "\n")
        if self.have_tracers:
            counts = [p["particles"] for p in parts]
            with open(os.path.join(t, "Particles", "Header"), "w") as f:
                f.write("castro_amd_particles_1\n%d\n%d\n" % (sum(counts), len(counts)) + "".join("%d\n" % c for c in counts))
        with open(os.path.join(t, STATE_FILE), "w") as f:
            json.dump(self.meta, f, indent=1, sort_keys=True)
            f.write("\n")

    # -- the thread ---------------------------------------------------------------------------------------------------------------
    def run(self, background):
        def body():
            try:
                if self.size == 1 and os.path.isdir(self.temp):
                    shutil.rmtree(self.temp)     # what an interrupted run left
                self.write_local()
                if self.size == 1:
                    self.finalize()             # no collective on one rank: the thread renames when it is done
            except BaseException as e:          # re-raised by wait()
                self.error = e
        if background:
            self.thread = threading.Thread(target=body, name="castro_amd-checkpoint", daemon=True)
            self.thread.start()
        else:
            body()

    def join(self):
        if self.thread is not None:
            self.thread.join()
            self.thread = None

    def wait(self):
        """join the thread, finish what it must not do itself, re-raise what it raised"""
        self.join()
        if self.size > 1:
            self.finalize()
        elif self.error is not None:
            err, self.error = self.error, None
            raise err


def _geom_line(geom, n_cell, l):
    r = 2 ** l
    plo, phi = [geom.problo[d] for d in range(3)], [geom.probhi[d] for d in range(3)]
    dom = PF._box((0, 0, 0), tuple(r * n_cell[d] - 1 for d in range(3)))
    per = [int(geom.lo_bc[d] == 0 and geom.hi_bc[d] == 0) for d in range(3)]
    return "%d ((%s,%s,%s) (%s,%s,%s)) %s %d %d %d\n" % ((geom.coord,) + tuple(_g(x) for x in plo + phi) + (dom,) + tuple(per))


def _header_text(run, levels, types):
    amr = _is_amr(run)
    max_level = run.max_level if amr else 0
    finest = len(levels) - 1
    g0, n_cell = levels[0]["geom"], run.n_cell
    nl = max_level + 1
    dt_level = [run.dt_level[l] for l in range(nl)] if amr else [run.dt]
    level_count = [run.level_count[l] for l in range(nl)] if amr else [0]
    out = [HEADER_VERSION + "\n", "3\n", _g(run.time) + "\n", "%d\n" % max_level, "%d\n" % finest]
    out += [_geom_line(g0, n_cell, l) for l in range(nl)]
    out.append("".join("2 " for _ in range(max_level)) + "\n")
    out.append("".join(_g(x) + " " for x in dt_level) + "\n")
    out.append("".join(_g(x) + " " for x in dt_level) + "\n")                      # dt_min: not tracked, dt_level again
    out.append("".join("%d " % (1 if l == 0 else 2) for l in range(nl)) + "\n")   # n_cycle
    out.append("".join("%d " % (run.nstep * 2 ** l) for l in range(nl)) + "\n")   # level_steps
    out.append("".join("%d " % c for c in level_count) + "\n")
    for l, lev in enumerate(levels):
        out.append("%d\n" % l)
        out.append("(%d 0\n" % len(lev["boxes"]) + "".join(PF._box(lo, hi) + "\n" for lo, hi in lev["boxes"]) + ")\n")
        out.append("%d\n" % len(types))
        dom = PF._box((0, 0, 0), tuple((2 ** l) * n_cell[d] - 1 for d in range(3)))
        dtl = dt_level[l]
        for k, nc in types:
            out.append("%d %d\n%s\n%s\n%s\n1\nLevel_%d/SD_%d_New_MF\n" % (k, nc, dom, _g(run.time - dtl), _g(run.time), l, k))
    return "".join(out)


def _job_info(run):
    lev0 = run.lev[0] if _is_amr(run) else run
    return PF.job_info_text(_comm(run).size, run.n_cell, run.nstep, run.time, lev0.geom, run.params)


def _driver_state(run):
    """castro_amd_state.json: what AMReX's Header has no slot for"""
    amr = _is_amr(run)
    comm = _comm(run)
    hydro = _hydro(run)
    st = dict(driver="CastroAmr" if amr else "Castro", nranks=comm.size, n_cell=list(run.n_cell), nstep=int(run.nstep),
              time=_hex(run.time), numerics=getattr(hydro, "numerics", None), have_sources=_have_sources(run),
              tracers=getattr(run, "tracers", None) is not None)
    pm = getattr(run, "pm", None)
    if pm is not None:
        st["point_mass_nupdates"] = int(pm.nupdates)
    if amr:
        st.update(dt_level=[_hex(x) for x in run.dt_level], level_count=[int(x) for x in run.level_count], nregrid=int(run.nregrid),
                  levels=[dict(lastDt=_hex(lev.lastDt), cached_est=_hex(getattr(lev, "_cached_est", None)),
                               post_clean_done=bool(lev._post_clean_done), nsubcycles=int(lev.nsubcycles)) for lev in run.lev])
    else:
        st.update(grid=list(run.grid), dt=_hex(run.dt), lastDt=_hex(run.lastDt), next_est=_hex(getattr(run, "_next_est", None)),
                  nsubcycles=int(run.nsubcycles))
    return st


# ---- reading ------------------------------------------------------------------------------------------------------------------
def _numbers(line):
    return re.findall(r"[-+]?(?:\d+\.?\d*(?:[eE][-+]?\d+)?|inf|nan)", line)


def read_header(dirname):
    """the text files of a checkpoint: dict(version, state_names, time, max_level, finest_level, geoms, dt_level, level_count,
    level_steps, levels=[dict(boxes, types=[(k, ncomp, path)])], point_mass, driver, particles)"""
    def text(name):
        with open(os.path.join(dirname, name)) as f:
            return f.read()
    head = text("CastroHeader").split()
    out = dict(version=int(head[-1]) if head and head[-1].lstrip("-").isdigit() else None,
               state_names=text("state_names.txt").split("\n")[:-1])
    H = text("Header").split("\n")
    if H[0] != HEADER_VERSION:
        raise ValueError("%s: the Header starts with %r, not %r" % (dirname, H[0], HEADER_VERSION))
    out["time"], out["max_level"], out["finest_level"] = float(H[2]), int(H[3]), int(H[4])
    nl = out["max_level"] + 1
    geoms = []
    for l in range(nl):
        v = _numbers(H[5 + l])
        geoms.append(dict(coord=int(v[0]), prob_lo=[float(x) for x in v[1:4]], prob_hi=[float(x) for x in v[4:7]],
                          dom_lo=[int(x) for x in v[7:10]], dom_hi=[int(x) for x in v[10:13]], periodic=[int(x) for x in v[16:19]]))
    out["geoms"] = geoms
    q = 5 + nl
    out["ref_ratio"] = [int(x) for x in H[q].split()]
    out["dt_level"] = [float(x) for x in H[q + 1].split()]
    out["dt_min"] = [float(x) for x in H[q + 2].split()]
    out["n_cycle"] = [int(x) for x in H[q + 3].split()]
    out["level_steps"] = [int(x) for x in H[q + 4].split()]
    out["level_count"] = [int(x) for x in H[q + 5].split()]
    q += 6
    levels = []
    for l in range(out["finest_level"] + 1):
        assert int(H[q]) == l, "Header: level %d expected at line %d" % (l, q + 1)
        nb = int(H[q + 1].strip("(").split()[0])
        boxes = []
        for b in range(nb):
            v = [int(x) for x in re.findall(r"-?\d+", H[q + 2 + b])]
            boxes.append((tuple(v[0:3]), tuple(v[3:6])))
        q += 2 + nb + 1
        ntypes = int(H[q])
        q += 1
        types = []
        for _ in range(ntypes):
            k, nc = (int(x) for x in H[q].split())
            types.append((k, nc, H[q + 5]))
            q += 6
        levels.append(dict(boxes=boxes, types=types))
    out["levels"] = levels
    out["point_mass"] = PF.read_point_mass(dirname)
    with open(os.path.join(dirname, STATE_FILE)) as f:
        out["driver"] = json.load(f)
    out["particles"] = None
    ph = os.path.join(dirname, "Particles", "Header")
    if os.path.exists(ph):
        tok = text(os.path.join("Particles", "Header")).split()
        out["particles"] = dict(total=int(tok[1]), counts=[int(x) for x in tok[3:3 + int(tok[2])]])
    return out


def read_particles(dirname, rank, count):
    """(pos (3, n), r (3, n), ints (4, n), flags (2)) of one rank's particle file"""
    with open(os.path.join(dirname, "Particles", "DATA_%05d" % rank), "rb") as f:
        raw = f.read()
    n = int(count)
    assert len(raw) == 64 * n + 8, "Particles/DATA_%05d: %d bytes for %d particles" % (rank, len(raw), n)
    pos = np.frombuffer(raw, dtype="<f8", count=3 * n, offset=0).reshape(3, n).copy()
    r = np.frombuffer(raw, dtype="<f8", count=3 * n, offset=24 * n).reshape(3, n).copy()
    ints = np.frombuffer(raw, dtype="<i4", count=4 * n, offset=48 * n).reshape(4, n).copy()
    flags = np.frombuffer(raw, dtype="<i4", count=2, offset=64 * n).copy()
    return pos, r, ints, flags


def read_level_fabs(dirname, path, want=None):
    """(ncomp, [dict(lo, hi, file, offset, min, max, data)]) of the MultiFab `path` (as the Header names it); want(index, box):
    whether the FAB of that box is read (data is None otherwise)"""
    nc, boxes = PF.read_vismf_header(os.path.join(dirname, path + "_H"))
    levdir = os.path.dirname(os.path.join(dirname, path))
    for i, b in enumerate(boxes):
        b["data"] = None
        if want is None or want(i, b):
            b["data"] = PF.read_fab(os.path.join(levdir, b["file"]), b["offset"], b["lo"], b["hi"])
            assert b["data"].shape[0] == nc
    return nc, boxes


def read_checkpoint(dirname):
    """A checkpoint as numpy: the dict of read_header plus nstep, dt and per level `state` and `source` (lists of arrays
    (ncomp, nz, ny, nx) in the order of `boxes`; source is None without Source_Type data), `headers` (per state type index the
    box entries of its VisMF header: file, offset, min, max) and `particles` with the arrays of every rank."""
    out = read_header(dirname)
    drv = out["driver"]
    out["nstep"] = int(drv["nstep"])
    out["time"] = _unhex(drv["time"])
    out["dt"] = _unhex(drv["dt"]) if "dt" in drv else _unhex(drv["dt_level"][0])
    if "dt_level" in drv:
        out["dt_level"] = [_unhex(x) for x in drv["dt_level"]]
    for lev in out["levels"]:
        lev["state"], lev["source"], lev["headers"] = None, None, {}
        for k, nc, path in lev["types"]:
            _, boxes = read_level_fabs(dirname, path)
            assert [(b["lo"], b["hi"]) for b in boxes] == lev["boxes"], "%s: the box array differs from the Header's" % path
            lev["state" if k == STATE_TYPE else "source"] = [b.pop("data") for b in boxes]
            lev["headers"][k] = boxes
    if out["particles"] is not None:
        out["particles"]["ranks"] = [read_particles(dirname, r, c) for r, c in enumerate(out["particles"]["counts"])]
    return out


# ---- the calls of the drivers -----------------------------------------------------------------------------------------------
def write_checkpoint(dirname, run, background=False):
    """Write the checkpoint `dirname` of a Castro or CastroAmr.  Collective on more than one rank.  Joins a checkpoint still in
    flight first.  background: return once the snapshot is on its way to host memory; run.checkpoint_wait() joins."""
    wait(run)
    job = _Job(run, dirname)
    if job.size > 1:
        if job.rank == 0 and os.path.isdir(job.temp):
            shutil.rmtree(job.temp)             # what an interrupted run left; the threads of all ranks create it again
        job.comm.barrier()
    run._ckpt_job = job
    job.run(background)
    if not background:
        wait(run)
    return job.dirname


def wait(run):
    """join the checkpoint in flight, if any: checkpoint_wait(), close() and the next writeCheckpoint"""
    job = run.__dict__.get("_ckpt_job")
    if job is None:
        return
    run._ckpt_job = None
    job.wait()


def _check(cond, what):
    if not cond:
        raise ValueError("restart: " + what)


def _validate(ck, run, dirname):
    amr = _is_amr(run)
    _check(ck["version"] == CASTRO_VERSION, "%s has CastroHeader version %r, this code reads version %d"
           % (dirname, ck["version"], CASTRO_VERSION))
    _check(ck["state_names"] == list(PF.STATE_NAMES), "the state names differ: %r in the checkpoint, %r here"
           % (ck["state_names"], list(PF.STATE_NAMES)))
    g = (run.lev[0] if amr else run).geom
    cg = ck["geoms"][0]
    n_cell = [cg["dom_hi"][d] - cg["dom_lo"][d] + 1 for d in range(3)]
    _check(n_cell == list(run.n_cell) and cg["dom_lo"] == [g.domlo[d] for d in range(3)],
           "n_cell / domain differs: %r in the checkpoint, %r here" % (n_cell, list(run.n_cell)))
    _check(cg["prob_lo"] == [g.problo[d] for d in range(3)], "prob_lo differs: %r in the checkpoint, %r here"
           % (cg["prob_lo"], [g.problo[d] for d in range(3)]))
    _check(cg["prob_hi"] == [g.probhi[d] for d in range(3)], "prob_hi differs: %r in the checkpoint, %r here"
           % (cg["prob_hi"], [g.probhi[d] for d in range(3)]))
    per = [int(g.lo_bc[d] == 0 and g.hi_bc[d] == 0) for d in range(3)]
    _check(cg["periodic"] == per, "the periodicity differs: %r in the checkpoint, %r here" % (cg["periodic"], per))
    drv = ck["driver"]
    _check(drv["driver"] == ("CastroAmr" if amr else "Castro"), "the checkpoint was written by a %s" % drv["driver"])
    comm = _comm(run)
    _check(int(drv["nranks"]) == comm.size, "the number of ranks differs: %d in the checkpoint, %d here" % (drv["nranks"], comm.size))
    if not amr:
        _check(list(drv["grid"]) == list(run.grid), "the rank grid differs: %r in the checkpoint, %r here" % (drv["grid"], list(run.grid)))
    max_level = run.max_level if amr else 0
    _check(ck["finest_level"] <= max_level, "finest_level %d of the checkpoint is above max_level %d" % (ck["finest_level"], max_level))
    have = any(k == SOURCE_TYPE for k, _, _ in ck["levels"][0]["types"])
    _check(have == _have_sources(run), "the checkpoint has no Source_Type data and this run has source terms" if not have
           else "the checkpoint has Source_Type data and this run has no source terms")
    tr = getattr(run, "tracers", None)
    _check((ck["particles"] is not None) == (tr is not None), "tracer particles on one side only: %s in the checkpoint, %s here"
           % ("present" if ck["particles"] is not None else "absent", "present" if tr is not None else "absent"))
    if tr is not None:
        _check(ck["particles"]["total"] == tr.n, "%d tracer particles in the checkpoint, %d here" % (ck["particles"]["total"], tr.n))
    _check((ck["point_mass"] is not None) == (getattr(run, "pm", None) is not None), "use_point_mass on one side only")


def _load_levels(ck, run, dirname):
    """the FABs of this rank's boxes into S_new_b / new_source: one unpack per level"""
    hydro = _hydro(run)
    for l, (lev, cl) in enumerate(zip(_levels(run), ck["levels"])):
        _check(lev["boxes"] == cl["boxes"], "the boxes of level %d differ: %r in the checkpoint, %r here" % (l, cl["boxes"], lev["boxes"]))
        mine = dict(lev["mine"])
        specs, chunks = [], []
        for k, nc, path in cl["types"]:
            _, boxes = read_level_fabs(dirname, path, want=lambda i, b: i in mine)
            for i, b in sorted(mine.items()):
                t, box = _fab_of(b, k)
                specs.append((t, box, (tuple(b.lo), tuple(b.hi))))
                chunks.append(np.ascontiguousarray(boxes[i]["data"], dtype=np.float64).reshape(-1))
        if not specs:
            continue
        src = torch.from_numpy(np.concatenate(chunks)).to(hydro.device)
        unpack(hydro, specs, src)


def restart_from(dirname, run):
    """Put the state of the checkpoint `dirname` into `run`, an object made with the arguments of the run that wrote it;
    called instead of initData.  ValueError, naming what differs, when the checkpoint does not fit the object."""
    wait(run)
    dirname = dirname.rstrip("/")
    if not os.path.isdir(dirname):
        raise FileNotFoundError("restart: no checkpoint directory %s" % dirname)
    ck = read_header(dirname)
    _validate(ck, run, dirname)
    drv = ck["driver"]
    amr = _is_amr(run)
    if amr:
        if run.refine is not None:
            # the box lists come from the file: no clustering; the levels through the path a regrid takes
            run._drop_fine()
            for cl in ck["levels"][1:]:
                run._push_level([(tuple(x // 2 for x in lo), tuple(x // 2 for x in hi)) for lo, hi in cl["boxes"]])
        _check(len(run.lev) == len(ck["levels"]), "%d levels in the checkpoint, %d here" % (len(ck["levels"]), len(run.lev)))
    _load_levels(ck, run, dirname)
    time, nstep = _unhex(drv["time"]), int(drv["nstep"])
    if amr:
        run.invalidate_estimates()
        run.time, run.nstep = time, nstep
        run.dt_level = [_unhex(x) for x in drv["dt_level"]]
        run.level_count = [int(x) for x in drv["level_count"]]
        run.nregrid = int(drv["nregrid"])
        for lev, d in zip(run.lev, drv["levels"]):
            lev.time, lev.nstep = time, nstep
            lev.lastDt, lev._cached_est = _unhex(d["lastDt"]), _unhex(d["cached_est"])
            lev._post_clean_done, lev.nsubcycles = bool(d["post_clean_done"]), int(d["nsubcycles"])
    else:
        run.time, run.nstep = time, nstep
        run.dt, run.lastDt, run._next_est = _unhex(drv["dt"]), _unhex(drv["lastDt"]), _unhex(drv["next_est"])
        run.nsubcycles = int(drv["nsubcycles"])
        run._pending_cleans, run._post_clean_done = 2, False
    pm = getattr(run, "pm", None)
    if pm is not None:
        pm.buf[0] = ck["point_mass"]            # %.17g reads back to the same double
        pm.buf[1] = 0.0
        pm.nupdates = int(drv.get("point_mass_nupdates", 0))
    tr = getattr(run, "tracers", None)
    if tr is not None:
        rank = _comm(run).rank
        tr.restore(*read_particles(dirname, rank, ck["particles"]["counts"][rank]))
    run.diag.reset()                            # diag_history starts empty; the logs are appended to (time > 0: no header)
    with open(os.path.join(dirname, "CPUtime")) as f:
        run._cpu_time_base = float(f.read().split()[0])
    run._wall_start = _time.perf_counter()
    run._last_check = nstep
    _comm(run).barrier()
    return ck


class CheckpointMixin:
    """writeCheckpoint / restart / checkpoint_wait and the amr.check_int trigger of Castro and CastroAmr"""

    check_int, check_file = -1, "chk"

    def writeCheckpoint(self, dirname=None, background=False):
        """Castro::checkPoint under Amr::checkPoint: the directory check_file + "%05d" % nstep (or `dirname`).  Collective on
        more than one rank: every rank writes its own boxes, rank 0 the text files; the rename follows a barrier.
        background=True: the pack launch and an asynchronous copy to pinned host memory are queued and the call returns; one
        thread writes the files; checkpoint_wait(), close() and the next writeCheckpoint join it and re-raise what it raised."""
        self._refuse_poisson("writeCheckpoint")
        if dirname is None:
            dirname = "%s%05d" % (self.check_file, self.nstep)
        self._last_check = self.nstep
        return write_checkpoint(dirname, self, background=background)

    def _checkpoint_join_only(self):
        """a finaliser's part: join the writer thread of a checkpoint in flight; no collective, nothing raised"""
        job, self._ckpt_job = self.__dict__.get("_ckpt_job"), None
        if job is not None:
            job.join()

    def checkpoint_wait(self):
        """join the background checkpoint, if one is in flight (collective on more than one rank)"""
        wait(self)

    def restart(self, dirname):
        """Castro::restart: instead of initData, on an object made with the arguments of the run that wrote `dirname`"""
        self._refuse_poisson("restart")
        return restart_from(dirname, self)

    def _refuse_poisson(self, what):
        from .gravity import PoissonGravity
        if isinstance(getattr(self, "gravity", None), PoissonGravity):      # Castro and CastroAmr keep their object there
            raise NotImplementedError("%s with Poisson gravity: a bit-faithful restart needs phi, the solver's starting guess, in "
                                      "the checkpoint (the reference's SD_1) -- a follow-up" % what)

    def _checkpoint_due(self):
        return self.check_int > 0 and self.nstep % self.check_int == 0 and self.__dict__.get("_last_check") != self.nstep

    def _checkpoint_cap(self, k):
        """the longest batch of host-free steps that does not run past the next checkpoint (DiagLog.cap for check_int)"""
        if self.check_int <= 0:
            return k
        return min(k, self.check_int - self.nstep % self.check_int)

    def _checkpoint_post_timestep(self):
        """evolve, after a coarse step or a batch: nstep % check_int == 0 writes chkNNNNN in the background"""
        if self._checkpoint_due():
            self.writeCheckpoint(background=True)

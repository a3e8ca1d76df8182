"""Tracer particles (castro.do_tracer_particles): Lagrangian fluid elements advected with the flow, for thermodynamic histories.

Reference: Source/particles/CastroParticles.cpp and its call sites -- init_particles (Castro.cpp:1399), advance_particles
(Castro_advance.cpp:115), the Redistribute / Timestamp of post_timestep (Castro.cpp:1982-1997) and of post_regrid (:2114-2117).
The container itself is AMReX's AmrTracerParticleContainer [3P, not in the reference tree]: AdvectWithUcc, Redistribute and the
cloud-in-cell interpolation are restated from its published algorithm (DESIGN.md "Tracer particles"); parity with an AMReX build
is unpinned.

`TracerParticles` spans the levels of a run like `MonopoleGravity`: it owns the particle arrays on the device (structure of
arrays; on one rank in id order, which never changes), two device flags and the timestamp file; `Castro(tracers=...)` and
`CastroAmr(tracers=...)` call it at the reference's call sites.  The four device operations are the backend's tracer_advect /
tracer_locate / tracer_sample / tracer_count (castro_amd/hydro.py over castro_amd/csrc/tracer_kernels.hip).

More than one rank (DESIGN.md "Tracer particles", ownership).  Every rank holds the particles of the boxes it owns, in arrays
sized exactly (n_local, possibly 0); `grid` stays the index in the level's global box list and every rank knows all boxes.
init_particles puts all N on rank 0; every Redistribute then ends with a migration: the backend's tracer_migrate_count (the
destination of every local particle and the counts per destination -- read on the host, the one synchronisation of a multi-rank
Redistribute: the receive sizes cannot be known without it), the counts of all ranks through comm.gather_objects,
tracer_migrate_pack (a stable partition: stayers into new arrays, leavers into 64-byte wire records), comm.exchange (one
message per non-empty pair of ranks) and tracer_unpack per source.  The order afterwards is defined: the stayers in their
previous order, then the arrivals by ascending source rank, each group in its order at the source -- two runs give identical
arrays.  Invalid particles and particles no box took stay where they are.  Reading particles back (positions(), ids(), ...,
write_ascii, the timestamp file) is collective: every rank gets all N in id order, rank 0 writes the files, line for line what
one rank writes.  check_flags sums the counts over the ranks, so that all ranks raise together.  A backend without the three
migration operations cannot run on more than one rank: bind() raises NotImplementedError.

Flags.  A particle whose interpolation stencil left the array it reads (impossible with CFL <= 1) is clamped by the kernel and
counted; a particle no box takes is counted too.  The counts are read once per step() of a run with tracers and wherever particle
data are read back, and either one raises RuntimeError.

Files.  `particle_init_file` is AMReX's ASCII form: N, then N lines `x y z`.  write_ascii writes N, then `x y z r0 r1 r2 id cpu`
per valid particle.  With timestamp_dir every Timestamp call appends one line per valid particle to timestamp_dir/Timestamp_00:
`id cpu x y z time [rho] [T]`, space separated, reals with 17 significant digits (file name and number format are this project's).

Restart.  A checkpoint holds every rank's pos, r, ints and the two flag words (castro_amd/checkpoint.py, Particles/); restore()
puts them back in place of init_particles.

Left out: total_particle_count, the binary particle directory of a plotfile, particle_restart_file, multi-rank AMR plotfiles."""
import os

import numpy as np
import torch

from . import _lib as L


MIGRATE_OPS = ("tracer_migrate_count", "tracer_migrate_pack", "tracer_unpack")
WIRE_TAG = 7001             # the tag of the particle records in comm.exchange


def can_migrate(hydro):
    """the backend has the three operations a run on more than one rank needs"""
    return all(hasattr(hydro, k) for k in MIGRATE_OPS)


def need_migration(hydro, comm):
    """the capability check of the constructors: looks at comm.size only"""
    if comm is not None and comm.size > 1 and not can_migrate(hydro):
        raise NotImplementedError("tracer particles on more than one rank need the migration between ranks, which is not built "
                                  "for this backend")


class _Arrays:
    """particle arrays a migration fills: what the backend's operations take in place of a TracerParticles"""

    def __init__(self, n, device):
        self.pos = torch.empty((3, n), dtype=torch.float64, device=device)
        self.r = torch.empty((3, n), dtype=torch.float64, device=device)
        self.ints = torch.empty((4, n), dtype=torch.int32, device=device)
        self._struct = None

    def struct(self):
        if self._struct is None:
            self._struct = L.make_tracers(self.pos, self.r, self.ints)
        return self._struct


def read_init_file(path):
    """positions (N, 3) of a particle_init_file"""
    with open(path) as f:
        tok = f.read().split()
    if not tok:
        raise ValueError("particle_init_file %s is empty" % path)
    n = int(tok[0])
    if n < 0 or len(tok) < 1 + 3 * n:
        raise ValueError("particle_init_file %s: %d particles announced, %d numbers follow" % (path, n, len(tok) - 1))
    return np.array([float(x) for x in tok[1:1 + 3 * n]], dtype=np.float64).reshape(n, 3)


class TracerParticles:
    def __init__(self, positions=None, init_file=None, timestamp_dir=None, timestamp_density=True, timestamp_temperature=False):
        """positions: float64 (N, 3), or init_file: a particle_init_file -- exactly one of the two.  timestamp_dir
        (castro.timestamp_dir): where Timestamp_00 is appended to; timestamp_density / timestamp_temperature
        (castro.timestamp_density, default 1 / castro.timestamp_temperature, default 0): the sampled fields."""
        if (positions is None) == (init_file is None):
            raise ValueError("TracerParticles takes either positions or init_file")
        if init_file is not None:
            positions = read_init_file(init_file)
        positions = np.array(positions, dtype=np.float64)
        if positions.ndim != 2 or positions.shape[1] != 3:
            raise ValueError("tracer positions must have shape (N, 3), not %s" % (positions.shape,))
        if not np.isfinite(positions).all():
            raise ValueError("tracer positions must be finite")
        self.initial_positions = positions
        self.n = positions.shape[0]
        self.timestamp_dir = timestamp_dir
        self.timestamp_comps = ([L.URHO] if timestamp_density else []) + ([L.UTEMP] if timestamp_temperature else [])
        self.hydro, self.pos, self.r, self.ints, self.flags, self._struct = None, None, None, None, None, None
        self.comm = None            # the communicator of a run on more than one rank, else None

    # ---- set-up --------------------------------------------------------------------------------------------------------------------
    def bind(self, hydro, geom, comm):
        """called by the driver that takes this object: the context the particle kernels run in and the domain check"""
        need_migration(hydro, comm)
        self.comm = comm if comm is not None and comm.size > 1 else None
        if not all(hasattr(hydro, k) for k in ("tracer_advect", "tracer_locate", "tracer_sample", "tracer_count")):
            raise RuntimeError("castro_amd: this backend has no tracer kernels; there is no host fallback")
        self.hydro = hydro
        self.check_domain(geom)

    def check_domain(self, geom):
        p = self.initial_positions
        for d in range(3):
            if geom.lo_bc[d] == 0 and geom.hi_bc[d] == 0:
                continue
            bad = ~((p[:, d] >= geom.problo[d]) & (p[:, d] < geom.probhi[d]))
            if bad.any():
                raise ValueError("tracer particle %d starts outside the domain in the non-periodic direction %s: %r"
                                 % (int(np.nonzero(bad)[0][0]) + 1, "xyz"[d], tuple(p[np.nonzero(bad)[0][0]])))

    def init_particles(self, geom):
        """Castro::init_particles: the particles of the input on level 0, ids 1..N in input order, cpu 0; the driver runs
        Redistribute(0) once its levels exist.  On more than one rank, rank 0 holds them all until then."""
        self.check_domain(geom)
        dev, n = self.hydro.device, self.n
        p0 = self.initial_positions
        if self.comm is not None and self.comm.rank != 0:
            n, p0 = 0, p0[:0]
        self.pos = torch.from_numpy(np.ascontiguousarray(p0.T)).to(dev).contiguous()                           # x, y, z rows
        self.r = torch.zeros((3, n), dtype=torch.float64, device=dev)
        self.ints = torch.zeros((4, n), dtype=torch.int32, device=dev)                                         # id, cpu, level, grid
        self.ints[0] = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)
        self._struct = None
        if self.timestamp_dir is not None and (self.comm is None or self.comm.rank == 0):
            os.makedirs(self.timestamp_dir, exist_ok=True)
            open(self.timestamp_file, "w").close()

    def restore(self, pos, r, ints, flags):
        """restart (castro_amd/checkpoint.py): this rank's arrays as a checkpoint holds them -- pos, r float64 (3, n), ints int32
        (4, n), the two flag words -- in place of init_particles.  Ids were handed out by init_particles of the run that wrote
        the checkpoint; the timestamp file is appended to, not started again."""
        dev = self.hydro.device
        self.pos = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float64)).to(dev).contiguous()
        self.r = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float64)).to(dev).contiguous()
        self.ints = torch.from_numpy(np.ascontiguousarray(ints, dtype=np.int32)).to(dev).contiguous()
        self.flags = torch.from_numpy(np.ascontiguousarray(flags, dtype=np.int32)).to(dev).contiguous()
        self._struct = None
        if self.timestamp_dir is not None and (self.comm is None or self.comm.rank == 0):
            os.makedirs(self.timestamp_dir, exist_ok=True)

    timestamp_file = property(lambda self: os.path.join(self.timestamp_dir, "Timestamp_00"))

    def struct(self):
        """the castro_amd_tracers of the device arrays"""
        if self._struct is None:
            self._struct = L.make_tracers(self.pos, self.r, self.ints)
        return self._struct

    @property
    def n_local(self):
        """the particles this rank holds (all N on one rank)"""
        return self.n if self.pos is None else int(self.pos.shape[1])

    def _ready(self):
        if self.pos is None:
            raise RuntimeError("tracer particles: initData has not run")

    # ---- the device operations ---------------------------------------------------------------------------------------------------
    def advect(self, level, boxes, geom, dt, ng):
        """AdvectWithUcc(level, dt): boxes = make_tracer_boxes of the half-time state of the level's boxes; ng: the ghost zones
        the reference's FillPatch asks for (the iteration) -- the fill paths here fill all of them"""
        self._ready()
        for ipass in (0, 1):
            self.hydro.tracer_advect(level, boxes, geom, dt, ipass, self, self.flags, ng=ng)

    def redistribute(self, level_boxes, geoms, lev_min, lev_max=None, ngrow=0, owners=None):
        """Redistribute(lev_min, lev_max = finest, ngrow); level_boxes[l]: [(lo, hi)] of the valid boxes of level l -- all of
        them, whoever owns them; owners[l]: their ranks (a run on more than one rank: the particles then move to the rank that
        owns their box)"""
        self._ready()
        lev_max = len(level_boxes) - 1 if lev_max is None else lev_max
        self.hydro.tracer_locate(lev_min, lev_max, ngrow, level_boxes, geoms, self, self.flags)
        if self.comm is not None:
            self._migrate(owners)

    def _migrate(self, owners):
        """the particles to the ranks that own their boxes (module docstring); collective"""
        if owners is None or len(owners) == 0:
            raise ValueError("tracer particles on more than one rank: Redistribute needs the owners of the boxes")
        h, comm, dev = self.hydro, self.comm, self.pos.device
        size, me, n = comm.size, comm.rank, self.n_local
        dest = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        counts = torch.zeros(size, dtype=torch.int32, device=dev)
        h.tracer_migrate_count(owners, size, me, self, dest, counts)
        mine = counts.tolist()                                  # the one synchronisation: the sizes of what is sent
        table = comm.gather_objects(mine)                       # table[source][destination]
        if not any(table[s][d] for s in range(size) for d in range(size) if s != d):
            return                                              # nobody moves: the arrays are the partition already
        nkeep, nleave = mine[me], sum(mine) - mine[me]
        arrive = [(s, table[s][me]) for s in range(size) if s != me and table[s][me] > 0]
        new = _Arrays(nkeep + sum(c for _, c in arrive), dev)
        wire = torch.empty((nleave, 8), dtype=torch.int64, device=dev)
        h.tracer_migrate_pack(size, me, self, dest, new, wire)
        sends, at = [], 0
        for d in range(size):
            if d != me and mine[d] > 0:
                sends.append((d, WIRE_TAG, wire[at:at + mine[d]]))
                at += mine[d]
        bufs = [(s, torch.empty((c, 8), dtype=torch.int64, device=dev)) for s, c in arrive]
        comm.exchange(sends, [(s, WIRE_TAG, b) for s, b in bufs])
        at = nkeep
        for s, b in bufs:                                       # ascending source rank
            h.tracer_unpack(b, new, at)
            at += int(b.shape[0])
        self.pos, self.r, self.ints, self._struct = new.pos, new.r, new.ints, None

    def check_flags(self):
        """the clamp and lost counts since the last look (one copy to the host); RuntimeError if either is set.  On more than
        one rank the counts are summed over the ranks first (collective): every rank raises, or none"""
        if self.flags is None:
            return
        if self.comm is not None:
            self.comm.allreduce_sum(self.flags)
        clamped, lost = self.flags.tolist()
        if clamped or lost:
            self.flags.zero_()
            what = []
            if clamped:
                what.append("%d particle passes had to clamp their interpolation stencil to the array (a particle moved more than "
                            "its ghost zones allow, or its box index is stale)" % clamped)
            if lost:
                what.append("%d lost particles (no box of any level holds them)" % lost)
            raise RuntimeError("tracer particles: " + "; ".join(what))

    def timestamp(self, lev_min, time, sample_boxes, geoms):
        """TimestampParticles: for every level >= lev_min that has valid particles, the timestamp components of the new-time
        state at that level's particles (sample_boxes(l): make_tracer_boxes of the ghost-filled S_new of level l), one line per
        particle appended to the timestamp file."""
        if self.timestamp_dir is None:
            return
        self._ready()
        if self.comm is not None:
            return self._timestamp_ranks(lev_min, time, sample_boxes, geoms)
        ints = self.ints.cpu().numpy()
        pos = self.pos.cpu().numpy()
        self.check_flags()
        nc = len(self.timestamp_comps)
        lines = []
        for l in range(lev_min, len(geoms)):
            sel = np.nonzero((ints[0] > 0) & (ints[2] == l))[0]
            if sel.size == 0:
                continue
            vals = None
            if nc:
                out = torch.zeros((nc, self.n), dtype=torch.float64, device=self.hydro.device)
                self.hydro.tracer_sample(l, sample_boxes(l), geoms[l], self.timestamp_comps, self, out, self.flags)
                vals = out.cpu().numpy()
                self.check_flags()
            for t in sel:
                f = ["%d" % ints[0, t], "%d" % ints[1, t]] + ["%.17g" % v for v in (pos[0, t], pos[1, t], pos[2, t], time)]
                f += ["%.17g" % vals[c, t] for c in range(nc)]
                lines.append(" ".join(f) + "\n")
        if lines:
            with open(self.timestamp_file, "a") as f:
                f.writelines(lines)

    def _timestamp_ranks(self, lev_min, time, sample_boxes, geoms):
        """timestamp() on more than one rank: every rank samples at its own particles, rank 0 writes the lines of all ranks in
        the order of one rank (per level, ascending id).  Collective; the same calls on every rank whatever it holds."""
        ints = self.ints.cpu().numpy()
        pos = self.pos.cpu().numpy()
        nc, n = len(self.timestamp_comps), self.n_local
        rows = []                                               # (level, id, line)
        for l in range(lev_min, len(geoms)):
            sel = np.nonzero((ints[0] > 0) & (ints[2] == l))[0]
            if sel.size == 0:
                continue
            vals = None
            if nc:
                out = torch.zeros((nc, n), dtype=torch.float64, device=self.pos.device)
                self.hydro.tracer_sample(l, sample_boxes(l), geoms[l], self.timestamp_comps, self, out, self.flags)
                vals = out.cpu().numpy()
            for t in sel:
                f = ["%d" % ints[0, t], "%d" % ints[1, t]] + ["%.17g" % v for v in (pos[0, t], pos[1, t], pos[2, t], time)]
                f += ["%.17g" % vals[c, t] for c in range(nc)]
                rows.append((l, int(ints[0, t]), " ".join(f) + "\n"))
        self.check_flags()
        rows = [r for part in self.comm.gather_objects(rows) for r in part]
        if rows and self.comm.rank == 0:
            rows.sort(key=lambda r: (r[0], r[1]))
            with open(self.timestamp_file, "a") as f:
                f.writelines(r[2] for r in rows)

    def count_level(self, level, box_list, geom, mine=None):
        """ParticleDerive: the number of valid particles of `level` in every zone of its boxes [(lo, hi)], as float64 tensors
        (nz, ny, nx) -- counted with integer atomics into int32 FABs, converted afterwards.  mine[b]: this rank owns box b (all
        of them by default); the others get no FAB and None in the result -- their particles are on their owners"""
        self._ready()
        h = self.hydro
        mine = [True] * len(box_list) if mine is None else list(mine)
        cnt = [torch.zeros(tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0)), dtype=torch.int32, device=h.device) if m else None
               for (lo, hi), m in zip(box_list, mine)]
        h.tracer_count(level, h.make_tracer_boxes([(lo, hi, None if c is None else (c, (lo, hi))) for c, (lo, hi) in zip(cnt, box_list)]),
                       geom, self)
        return [None if c is None else c.to(torch.float64) for c in cnt]

    # ---- read-back ---------------------------------------------------------------------------------------------------------------
    def _host(self):
        """(pos, r, ints) of all particles on the host, in id order; collective on more than one rank"""
        self._ready()
        out = self.pos.cpu().numpy(), self.r.cpu().numpy(), self.ints.cpu().numpy()
        if self.comm is not None:
            parts = self.comm.gather_objects(out)
            out = tuple(np.concatenate([p[k] for p in parts], axis=1) for k in range(3))
            order = np.argsort(np.abs(out[2][0]), kind="stable")            # an invalid particle carries -id
            out = tuple(np.ascontiguousarray(a[:, order]) for a in out)
        self.check_flags()
        return out

    def positions(self):
        """(N, 3) positions of all particles, invalid ones included, in id order"""
        return self._host()[0].T.copy()

    def velocities(self):
        """(N, 3): r0..r2 -- after an advance the velocity its corrector used"""
        return self._host()[1].T.copy()

    def ids(self):
        """id per particle: 1..N, negated once the particle has left the domain"""
        return self._host()[2][0].copy()

    def levels(self):
        return self._host()[2][2].copy()

    def grids(self):
        return self._host()[2][3].copy()

    @property
    def num_valid(self):
        return int((self._host()[2][0] > 0).sum())

    def write_ascii(self, path):
        """N, then `x y z r0 r1 r2 id cpu` per valid particle (reals with 17 significant digits); on more than one rank
        collective, written by rank 0"""
        pos, r, ints = self._host()
        if self.comm is not None and self.comm.rank != 0:
            return
        sel = np.nonzero(ints[0] > 0)[0]
        with open(path, "w") as f:
            f.write("%d\n" % sel.size)
            for t in sel:
                f.write(" ".join(["%.17g" % v for v in (pos[0, t], pos[1, t], pos[2, t], r[0, t], r[1, t], r[2, t])]
                                 + ["%d" % ints[0, t], "%d" % ints[1, t]]) + "\n")

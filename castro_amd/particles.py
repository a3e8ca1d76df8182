"""Tracer particles (castro.do_tracer_particles): Lagrangian fluid elements advected with the flow, for thermodynamic histories.

Reference: Source/particles/CastroParticles.cpp and its call sites -- init_particles (Castro.cpp:1399), advance_particles
(Castro_advance.cpp:115), the Redistribute / Timestamp of post_timestep (Castro.cpp:1982-1997) and of post_regrid (:2114-2117).
The container itself is AMReX's AmrTracerParticleContainer [3P, not in the reference tree]: AdvectWithUcc, Redistribute and the
cloud-in-cell interpolation are restated from its published algorithm (DESIGN.md "Tracer particles"); parity with an AMReX build
is unpinned.

`TracerParticles` spans the levels of a run like `MonopoleGravity`: it owns the particle arrays on the device (structure of
arrays, in id order, which never changes), two device flags and the timestamp file; `Castro(tracers=...)` and
`CastroAmr(tracers=...)` call it at the reference's call sites.  The four device operations are the backend's tracer_advect /
tracer_locate / tracer_sample / tracer_count (castro_amd/hydro.py over castro_amd/csrc/tracer_kernels.hip).

Flags.  A particle whose interpolation stencil left the array it reads (impossible with CFL <= 1) is clamped by the kernel and
counted; a particle no box takes is counted too.  The counts are read once per step() of a run with tracers and wherever particle
data are read back, and either one raises RuntimeError.

Files.  `particle_init_file` is AMReX's ASCII form: N, then N lines `x y z`.  write_ascii writes N, then `x y z r0 r1 r2 id cpu`
per valid particle.  With timestamp_dir every Timestamp call appends one line per valid particle to timestamp_dir/Timestamp_00:
`id cpu x y z time [rho] [T]`, space separated, reals with 17 significant digits (file name and number format are this project's).

Left out: total_particle_count, the binary particle directory of a plotfile, restart, more than one rank."""
import os

import numpy as np
import torch

from . import _lib as L


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

    # ---- set-up --------------------------------------------------------------------------------------------------------------------
    def bind(self, hydro, geom, comm):
        """called by the driver that takes this object: the context the particle kernels run in and the domain check"""
        if comm is not None and comm.size > 1:
            raise NotImplementedError("tracer particles on more than one rank need the migration between ranks, which is not built")
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
        Redistribute(0) once its levels exist"""
        self.check_domain(geom)
        dev, n = self.hydro.device, self.n
        self.pos = torch.from_numpy(np.ascontiguousarray(self.initial_positions.T)).to(dev).contiguous()       # x, y, z rows
        self.r = torch.zeros((3, n), dtype=torch.float64, device=dev)
        self.ints = torch.zeros((4, n), dtype=torch.int32, device=dev)                                         # id, cpu, level, grid
        self.ints[0] = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)
        self._struct = None
        if self.timestamp_dir is not None:
            os.makedirs(self.timestamp_dir, exist_ok=True)
            open(self.timestamp_file, "w").close()

    timestamp_file = property(lambda self: os.path.join(self.timestamp_dir, "Timestamp_00"))

    def struct(self):
        """the castro_amd_tracers of the device arrays"""
        if self._struct is None:
            self._struct = L.make_tracers(self.pos, self.r, self.ints)
        return self._struct

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

    def redistribute(self, level_boxes, geoms, lev_min, lev_max=None, ngrow=0):
        """Redistribute(lev_min, lev_max = finest, ngrow); level_boxes[l]: [(lo, hi)] of the valid boxes of level l"""
        self._ready()
        lev_max = len(level_boxes) - 1 if lev_max is None else lev_max
        self.hydro.tracer_locate(lev_min, lev_max, ngrow, level_boxes, geoms, self, self.flags)

    def check_flags(self):
        """the clamp and lost counts since the last look (one copy to the host); RuntimeError if either is set"""
        if self.flags is None:
            return
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

    def count_level(self, level, box_list, geom):
        """ParticleDerive: the number of valid particles of `level` in every zone of its boxes [(lo, hi)], as float64 tensors
        (nz, ny, nx) -- counted with integer atomics into int32 FABs, converted afterwards"""
        self._ready()
        h = self.hydro
        cnt = [torch.zeros(tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0)), dtype=torch.int32, device=h.device) for lo, hi in box_list]
        h.tracer_count(level, h.make_tracer_boxes([(lo, hi, (c, (lo, hi))) for c, (lo, hi) in zip(cnt, box_list)]), geom, self)
        return [c.to(torch.float64) for c in cnt]

    # ---- read-back ---------------------------------------------------------------------------------------------------------------
    def _host(self):
        self._ready()
        out = self.pos.cpu().numpy(), self.r.cpu().numpy(), self.ints.cpu().numpy()
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
        """N, then `x y z r0 r1 r2 id cpu` per valid particle (reals with 17 significant digits)"""
        pos, r, ints = self._host()
        sel = np.nonzero(ints[0] > 0)[0]
        with open(path, "w") as f:
            f.write("%d\n" % sel.size)
            for t in sel:
                f.write(" ".join(["%.17g" % v for v in (pos[0, t], pos[1, t], pos[2, t], r[0, t], r[1, t], r[2, t])]
                                 + ["%d" % ints[0, t], "%d" % ints[1, t]]) + "\n")

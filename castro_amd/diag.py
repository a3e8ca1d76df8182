"""Host side of Castro::sum_integrated_quantities (Source/driver/sum_integrated_quantities.cpp): the dictionary made of the
14 sums of castro_amd_integrated_quantities_mf, the trigger of Castro::post_timestep (castro.sum_interval), and the data logs
grid_diag.out / species_diag.out / amr_diag.out in the reference's layout.  Shared by Castro and CastroAmr."""
import os
import time as _time

from . import _lib as L

# sum_integrated_quantities.cpp:45-49
DATPRECISION, DATWIDTH, FIXWIDTH, INTWIDTH = 16, 25, 25, 12

# grid_diag.out, in the reference's order: rho_K in front of rho_e (sum_integrated_quantities.cpp:176-215; the gravity
# columns rho_phi / total energy are filled for PoissonGrav only and are not written)
GRID_DIAG_COLUMNS = ("time", "mass", "xmom", "ymom", "zmom", "ang mom x", "ang mom y", "ang mom z", "rho_K", "rho_e", "rho_E")
SPECIES_NAMES = ("X",)


def domain_center(castro):
    """problem::center as the plotfile derives take it: the `center` attribute of the driver, else the middle of the domain"""
    c = getattr(castro, "center", None)
    g = castro.geom
    return [0.5 * (g.problo[d] + g.probhi[d]) for d in range(3)] if c is None else list(c)


def quantities(time, v):
    """the dictionary of sum_integrated_quantities from the CASTRO_AMD_DIAG_N sums `v` (a list of floats)"""
    mass = v[L.DIAG_MASS]
    mom = [v[L.DIAG_XMOM], v[L.DIAG_YMOM], v[L.DIAG_ZMOM]]
    inv = (1.0 / mass) if mass != 0.0 else float("nan")
    return dict(time=time, mass=mass, mom=mom,
                ang_mom=[v[L.DIAG_ANGMOM_X], v[L.DIAG_ANGMOM_Y], v[L.DIAG_ANGMOM_Z]],
                rho_e=v[L.DIAG_RHO_E_INT], rho_K=v[L.DIAG_RHO_K], rho_E=v[L.DIAG_RHO_E],
                com=[v[L.DIAG_COM_X + d] * inv if mass != 0.0 else float("nan") for d in range(3)],
                com_vel=[mom[d] * inv if mass != 0.0 else float("nan") for d in range(3)],
                species_mass=[v[L.DIAG_SPECIES] / L.M_SOLAR])


def grid_diag_row(q):
    return [q["time"], q["mass"]] + list(q["mom"]) + list(q["ang_mom"]) + [q["rho_K"], q["rho_e"], q["rho_E"]]


def _sci(x):
    return "%*.*e" % (DATWIDTH, DATPRECISION, x)


def _fix(x):
    return "%*.*f" % (FIXWIDTH, DATPRECISION, x)


class DiagLog:
    """castro.sum_interval, castro.show_center_of_mass and the three data logs.  One per driver object: it keeps the history,
    decides when a sum is due and appends the rows (the I/O rank only; a directory of None writes nothing)."""

    def __init__(self, sum_interval=-1, show_center_of_mass=False, diag_dir=None, io_rank=True):
        self.sum_interval = int(sum_interval)
        self.show_center_of_mass = bool(show_center_of_mass)
        self.diag_dir, self.io_rank = diag_dir, bool(io_rank)
        self.history = []
        self.last_nstep = None
        self.wall_start, self.wall_steps = None, 1

    # ---- the trigger (Castro::post_timestep: nstep % sum_interval == 0; post_init: always) --------------------------
    def due(self, nstep):
        return self.sum_interval > 0 and nstep % self.sum_interval == 0 and self.last_nstep != nstep

    def cap(self, k, nstep):
        """the longest batch of host-free steps from step count `nstep` that does not run past the next sum"""
        if self.sum_interval <= 0:
            return k
        return min(k, self.sum_interval - nstep % self.sum_interval)

    def begin_steps(self, nsteps=1):
        """called in front of a coarse step (or a batch of them): the wall clock of amr_diag.out"""
        if self.sum_interval > 0:
            self.wall_start, self.wall_steps = _time.perf_counter(), max(int(nsteps), 1)

    def reset(self):
        self.history, self.last_nstep = [], None

    # ---- one entry ------------------------------------------------------------------------------------------------
    def record(self, q, nstep, dt, finest_level=0):
        """append the entry of step `nstep` (q: quantities()) to the history and to the logs"""
        wall = 0.0
        if q["time"] > 0.0 and self.wall_start is not None:
            wall = (_time.perf_counter() - self.wall_start) / self.wall_steps
        q = dict(q, nstep=int(nstep), dt=float(dt), finest_level=int(finest_level), wall_time=wall)
        self.history.append(q)
        self.last_nstep = int(nstep)
        if self.show_center_of_mass and self.io_rank:
            for d, ax in enumerate("XYZ"):
                print("TIME= %r CENTER OF MASS %s-LOC = %r" % (q["time"], ax, q["com"][d]))
                print("TIME= %r CENTER OF MASS %s-VEL = %r" % (q["time"], ax, q["com_vel"][d]))
        if self.diag_dir is not None and self.io_rank:
            self.write(q)
        return q

    def write(self, q):
        first = q["time"] == 0.0
        os.makedirs(self.diag_dir, exist_ok=True)
        mode = "w" if first else "a"
        with open(os.path.join(self.diag_dir, "grid_diag.out"), mode) as f:
            if first:
                f.write("".join("%*s" % (DATWIDTH, "%14s" % c) for c in GRID_DIAG_COLUMNS) + "\n")
            f.write("".join(_sci(x) for x in grid_diag_row(q)) + "\n")
        with open(os.path.join(self.diag_dir, "species_diag.out"), mode) as f:
            if first:
                n = 2 + len(SPECIES_NAMES)
                f.write("%*s%*s" % (INTWIDTH, "#   COLUMN 1", FIXWIDTH, "2") + "".join("%*d" % (DATWIDTH, i) for i in range(3, n + 1)) + "\n")
                f.write("%*s%*s" % (INTWIDTH, "#   TIMESTEP", FIXWIDTH, "TIME")
                        + "".join("%*s" % (DATWIDTH, "Mass " + s) for s in SPECIES_NAMES) + "\n")
            f.write("%*d" % (INTWIDTH, q["nstep"]) + _fix(q["time"]) + "".join(_sci(x) for x in q["species_mass"]) + "\n")
        with open(os.path.join(self.diag_dir, "amr_diag.out"), mode) as f:
            if first:
                f.write("%*s%*s%*d%*d%*d\n" % (INTWIDTH, "#   COLUMN 1", FIXWIDTH, "2", DATWIDTH, 3, INTWIDTH, 4, DATWIDTH, 5))
                f.write("%*s%*s%*s%*s%*s\n" % (INTWIDTH, "#   TIMESTEP", FIXWIDTH, "TIME", FIXWIDTH, "DT", INTWIDTH, "  FINEST LEV",
                                               FIXWIDTH, " COARSE TIMESTEP WALLTIME"))
            f.write("%*d" % (INTWIDTH, q["nstep"]) + _fix(q["time"]) + _fix(q["dt"]) + "%*d" % (INTWIDTH, q["finest_level"])
                    + _fix(q["wall_time"]) + "\n")


def read_grid_diag(path):
    """(column names, rows of floats) of a grid_diag.out: fixed columns of DATWIDTH characters, one header row"""
    with open(path) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip()]
    cut = lambda ln: [ln[i:i + DATWIDTH] for i in range(0, len(ln), DATWIDTH)]
    names = [c.strip() for c in cut(lines[0])]
    return names, [[float(c) for c in cut(ln)] for ln in lines[1:]]

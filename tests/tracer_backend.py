"""tests/oracle_backend.OracleBackend with the four tracer-particle operations from the numpy restatement (tests/tracer_ref.py),
so that Castro(tracers=...) and CastroAmr(tracers=...) run on the CPU.  Every call is logged (`calls`) so that a test can read
the schedule.  perturb: every half-time array an advection reads is multiplied by 1 + perturb * U(-1, 1) first (the sensitivity
run of the `contract` driver test).  Tests only."""
import numpy as np

from tests import tracer_ref as R
from tests.oracle_backend import OracleBackend


class TracerOracleBackend(OracleBackend):
    calls = None            # shared by the contexts of a hierarchy when the test sets it on the class or passes `calls`

    def __init__(self, *a, calls=None, perturb=0.0, seed=0, **k):
        super().__init__(*a, **k)
        self.calls = calls if calls is not None else []
        self.perturb, self._rng, self._noisy = float(perturb), np.random.default_rng(seed), None

    @staticmethod
    def _P(tr):
        """the restatement's particle dict as views of the driver's (CPU) tensors"""
        pos, r, ints = tr.pos.numpy(), tr.r.numpy(), tr.ints.numpy()
        return dict(x=pos[0], y=pos[1], z=pos[2], r0=r[0], r1=r[1], r2=r[2], id=ints[0], cpu=ints[1], level=ints[2], grid=ints[3])

    @staticmethod
    def make_tracer_boxes(specs):
        return [(fab[0].numpy(), (tuple(fab[1][0]), tuple(fab[1][1])), (tuple(vlo), tuple(vhi))) for vlo, vhi, fab in specs]

    def tracer_advect(self, level, boxes, geom, dt, ipass, tracers, flags, stream=None, ng=None):
        self.calls.append(("advect", level, ipass, ng))
        if self.perturb:
            if ipass == 0:
                self._noisy = [(fab * (1.0 + self.perturb * self._rng.uniform(-1.0, 1.0, size=fab.shape)), ab, vb)
                               for fab, ab, vb in boxes]
            boxes = self._noisy
        R.advect_pass(self._P(tracers), level, boxes, geom, dt, ipass, flags.numpy())

    def tracer_locate(self, lev_min, lev_max, ngrow, level_boxes, geoms, tracers, flags, stream=None):
        self.calls.append(("locate", lev_min, lev_max, ngrow))
        R.locate(self._P(tracers), lev_min, lev_max, ngrow, level_boxes, geoms, flags.numpy())

    def tracer_sample(self, level, boxes, geom, comps, tracers, out, flags, stream=None):
        self.calls.append(("sample", level, tuple(comps)))
        R.sample(self._P(tracers), level, boxes, geom, comps, out.numpy(), flags.numpy())

    def tracer_count(self, level, boxes, geom, tracers, stream=None):
        self.calls.append(("count", level))
        R.count(self._P(tracers), level, [(fab, ab) for fab, ab, _ in boxes], geom)

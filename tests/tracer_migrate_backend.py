"""tests/tracer_backend.TracerOracleBackend (left as it is) with the three migration operations from the numpy restatement
(tests/tracer_migrate_ref.py) and box tables that take entries without a FAB -- the boxes of other ranks -- so that
Castro(tracers=..., comm=DistComm()) and CastroAmr(tracers=..., comm=DistComm()) run on the CPU over gloo.  Tests only."""
import numpy as np

from tests import tracer_migrate_ref as M
from tests import tracer_ref as R
from tests.tracer_backend import TracerOracleBackend


class TracerMigrateOracleBackend(TracerOracleBackend):
    @staticmethod
    def make_tracer_boxes(specs):
        return [(None, None, (tuple(vlo), tuple(vhi))) if fab is None
                else (fab[0].numpy(), (tuple(fab[1][0]), tuple(fab[1][1])), (tuple(vlo), tuple(vhi))) for vlo, vhi, fab in specs]

    @staticmethod
    def _without_fabless(P, level, boxes, flags):
        """P with the particles of `level` whose grid names an entry without a FAB taken out of the level (a copy of `level`
        only: the other arrays stay views); each adds 1 to flags[0] when flags are given"""
        nofab = np.array([b[0] is None for b in boxes], dtype=bool)
        if not nofab.any():
            return P
        g = P["grid"]
        bad = (P["id"] > 0) & (P["level"] == level) & (g >= 0) & (g < len(boxes))
        bad[bad] = nofab[g[bad]]
        if flags is not None:
            flags[0] += int(bad.sum())
        Q = dict(P)
        Q["level"] = np.where(bad, -1, P["level"]).astype(np.int32)
        return Q

    def tracer_advect(self, level, boxes, geom, dt, ipass, tracers, flags, stream=None, ng=None):
        self.calls.append(("advect", level, ipass, ng))
        R.advect_pass(self._without_fabless(self._P(tracers), level, boxes, flags.numpy()), level, boxes, geom, dt, ipass, flags.numpy())

    def tracer_sample(self, level, boxes, geom, comps, tracers, out, flags, stream=None):
        self.calls.append(("sample", level, tuple(comps)))
        R.sample(self._without_fabless(self._P(tracers), level, boxes, flags.numpy()), level, boxes, geom, comps, out.numpy(), flags.numpy())

    def tracer_count(self, level, boxes, geom, tracers, stream=None):
        self.calls.append(("count", level))
        R.count(self._without_fabless(self._P(tracers), level, boxes, None), level, [(fab, ab) for fab, ab, _ in boxes], geom)

    # ---- migration -----------------------------------------------------------------------------------------------------------------
    def tracer_migrate_count(self, level_owners, nranks, myrank, tracers, dest, counts, stream=None):
        self.calls.append(("migrate_count", nranks, myrank))
        P = self._P(tracers)
        d, c = M.destinations(P, level_owners, nranks, myrank)
        dest.numpy()[:d.shape[0]] = d
        counts.numpy()[:nranks] = c

    def tracer_migrate_pack(self, nranks, myrank, tracers, dest, out, wire, stream=None):
        self.calls.append(("migrate_pack", nranks, myrank))
        P = self._P(tracers)
        kept, w = M.pack(P, dest.numpy()[:P["id"].shape[0]], nranks, myrank)
        Q, nk = self._P(out), kept["id"].shape[0]
        for k in Q:
            Q[k][:nk] = kept[k]
        wire.numpy()[:] = w

    def tracer_unpack(self, wire, out, at, stream=None):
        self.calls.append(("unpack", int(wire.shape[0]), at))
        M.unpack(wire.numpy(), self._P(out), at)

"""tests/oracle_backend.OracleBackend with the boundary overrides of the state fill: ext_bc_fill from the numpy restatement
(tests/ext_bc_ref.py), so that Castro(ext_bc=...) and CastroAmr(ext_bc=...) run on the CPU.  Tests only."""
from tests import ext_bc_ref as R
from tests.oracle_backend import OracleBackend


class ExtBcOracleBackend(OracleBackend):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ext_fills = 0

    def ext_bc_fill(self, state, box, geom, params, ext, unconverged=None, stream=None):
        self.ext_fills += 1
        bad = R.ext_bc_fill(state.numpy(), box, geom, params, ext)          # in place: numpy() shares the tensor's memory
        if unconverged is not None:
            unconverged += bad

"""CASTRO_AMD_OP_CLEAN of castro_amd_fab_ops_p against castro_amd_clean_state_fab, bit for bit in BOTH numerics builds.

A level with every box on one rank cleans its boxes through an operation table, a level whose boxes are dealt over ranks box
by box; runs on R ranks equal the one-rank run bit for bit only if the two forms give the same bits.  In the `contract` build
two compiled copies of clean_zone may contract differently, so the table hands its CLEAN operations to clean_state's own
kernel (castro_amd/csrc/aux_kernels.hip: launch_fab_ops)."""
import numpy as np
import pytest
import torch

from tests.util import physical_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["exact", "contract"])
def hydro(request):
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=request.param)
    yield h
    h.close()


@pytest.mark.parametrize("nbox", [1, 3, 20])        # one operation; a table in the kernel arguments; one in device memory (> 16)
@pytest.mark.parametrize("ntimes", [1, 2])
def test_clean_operations_of_a_table_equal_clean_state(hydro, nbox, ntimes):
    """rough states, a fifth of the densities under small_dens, rho X != rho, odd extents, a region inside the FAB: every
    component of every zone equal, the zones outside the region untouched"""
    import castro_amd
    from castro_amd import _lib as L
    rng = np.random.default_rng(4300 + nbox)
    P = castro_amd.default_params(small_dens=0.3)
    lo, hi = (2, 4, 6), (14, 12, 16)
    box = (tuple(x - 3 for x in lo), tuple(x + 3 for x in hi))
    one, tab, raw = [], [], []
    for _ in range(nbox):
        u = physical_state(rng, box[0], box[1], smooth=False)
        u[0] *= rng.uniform(0.2, 1.0, size=u[0].shape)
        raw.append(u)
        one.append(torch.from_numpy(np.ascontiguousarray(u)).to(hydro.device))
        tab.append(one[-1].clone())
    for t in one:
        hydro.clean_state(t, box, lo, hi, P, ntimes=ntimes)
    hydro.fab_ops(hydro.make_ops([(L.OP_CLEAN, 0, 8, lo, hi, float(ntimes), 0.0, (t, box), (t, box), None) for t in tab]), params=P)
    torch.cuda.synchronize()
    assert hydro.status() == 0
    for i in range(nbox):
        assert torch.equal(one[i], tab[i]), "box %d: %d values differ" % (i, int((one[i] != tab[i]).sum()))
    got = tab[0].cpu().numpy()
    inside = np.zeros(got.shape, dtype=bool)
    inside[:, 3:-3, 3:-3, 3:-3] = True
    assert np.array_equal(got[~inside], raw[0][~inside]) and (got[inside] != raw[0][inside]).any()

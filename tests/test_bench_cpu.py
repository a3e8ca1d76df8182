"""bench.py --dump-outputs without a GPU: which zones are written, and that the ranks' parts put back together are the global state."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_selection_is_fixed_in_range_and_within_64_mb():
    for n in ((16, 16, 16), (64, 64, 64), (96, 80, 128), (256, 256, 256), (512, 512, 512)):
        a, b = bench.dump_selection(n), bench.dump_selection(n)
        assert a.keys() == b.keys()
        total = 0
        for name, (k, j, i, shape) in a.items():
            assert all(np.array_equal(x, y) for x, y in zip((k, j, i), b[name][:3]))          # same zones from run to run
            assert k.min() >= 0 and k.max() < n[2] and j.min() >= 0 and j.max() < n[1] and i.min() >= 0 and i.max() < n[0]
            assert int(np.prod(shape)) == len(k)
            total += 8 * 8 * len(k)
        assert total <= 32 << 20
        whole = n[0] * n[1] * n[2] * 64 <= bench.DUMP_FULL_BYTES
        assert set(a) == ({"state"} if whole else {"state_center", "state_sample"})


def test_gathered_outputs_of_split_boxes_equal_the_global_state():
    """gather_outputs on every rank's box of a decomposed domain, reassembled as rank 0 does, against the global array"""
    for n, grid in (((16, 16, 16), (1, 1, 1)), ((32, 32, 32), (1, 1, 2)), ((96, 96, 96), (1, 2, 2)), ((100, 80, 120), (1, 1, 1))):
        G = torch.arange(8 * n[0] * n[1] * n[2], dtype=torch.float64).reshape(8, n[2], n[1], n[0])
        boxes = []
        for r in range(grid[0] * grid[1] * grid[2]):
            co = (r % grid[0], (r // grid[0]) % grid[1], r // (grid[0] * grid[1]))
            lo = tuple(co[d] * (n[d] // grid[d]) for d in range(3))
            hi = tuple(lo[d] + n[d] // grid[d] - 1 for d in range(3))
            boxes.append((G[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1], lo, hi))
        parts = []

        def driver(S, lo, hi, gather):
            return SimpleNamespace(S_new=lambda: S, lo=lo, hi=hi, dt=1.5e-3, time=0.25, comm=SimpleNamespace(gather_objects=gather))
        for S, lo, hi in boxes:                             # every rank's contribution
            bench.gather_outputs(driver(S, lo, hi, lambda obj: parts.append(obj) or [obj]), n)
        out = bench.gather_outputs(driver(*boxes[0], lambda obj: parts), n)
        assert out["dt"].tolist() == [1.5e-3] and out["time"].tolist() == [0.25]
        for name, (k, j, i, shape) in bench.dump_selection(n).items():
            want = G[:, torch.from_numpy(k), torch.from_numpy(j), torch.from_numpy(i)].numpy().reshape((8,) + shape)
            assert out[name].dtype == np.float64 and np.array_equal(out[name], want), (n, grid, name)

"""castro_amd -- MI355X-native CTU Godunov hydro advance for Castro (one hot path, C-ABI drop-in).

Layout:
  csrc/            hand-written HIP kernels for gfx950 + the C ABI (include/castro_hydro_amd.h)
  _lib.py          ctypes binding of libcastro_hydro_amd.so (no CPU fallback)
  hydro.py         HipHydro: the reference's per-FAB hydro interface over the C ABI
  castro.py        Castro: single-level driver (FillPatch halo exchange over RCCL, dt control, retry, gravity, rotation, thermal diffusion, sponge)
  amr.py           CastroAmr: coarse level + one refined patch with subcycling, reflux, avgDown
  gravity.py       MonopoleGravity: monopole self-gravity over the levels of CastroAmr (radial arrays, level combination); PointMass: the central point mass; PoissonGravity: Poisson self-gravity of a single level (multipole boundary values, multigrid) and of the levels of CastroAmr (level solves)
  particles.py     TracerParticles: tracer particles over the levels of Castro / CastroAmr (advect, redistribute, timestamp, particle_count)
  plotfile.py      Castro plotfile writer / reader
  checkpoint.py    checkpoint / restart of Castro and CastroAmr (write_checkpoint, restart_from, read_checkpoint)
"""
from ._lib import (NUM_STATE, NGDNV, NUM_GROW, URHO, UMX, UMY, UMZ, UEDEN, UEINT, UTEMP, UFS,
                   default_params, make_geom, make_rotation, make_diffusion, make_sponge, make_ext_bc, LIB_PATH)
from .castro import Castro, DistComm, SingleComm, AdvanceFailure, default_grid
from .amr import CastroAmr
from .gravity import MonopoleGravity, PointMass, PoissonGravity
from .particles import TracerParticles
from .checkpoint import read_checkpoint

__all__ = ["Castro", "CastroAmr", "read_checkpoint", "MonopoleGravity", "PointMass", "PoissonGravity", "TracerParticles", "DistComm", "SingleComm", "AdvanceFailure", "default_grid", "default_params", "make_geom", "make_rotation", "make_diffusion", "make_sponge", "make_ext_bc",
           "NUM_STATE", "NGDNV", "NUM_GROW", "LIB_PATH"]


def HipHydro(*a, **k):
    from .hydro import HipHydro as _H
    return _H(*a, **k)

#!/usr/bin/env python3
"""Time of one training inner-loop step -- accumulate (EnergyGradient) + one sweep (num_sites mc_steps), the body of
run_optimization_epoch (training.py:608-617) -- of the gnn ansatz on the general convolution path, next to conv_2d
on the same stencil through the general im2col path and through its default path.

  python tools/gnn_bench.py [--chains 1024] [--reps 5]

Host clock around synchronised work, after a warm-up; needs a GPU (fails without one).  One line per case.
For the gather kernels' share of the step, run it under `rocprofv3 --kernel-trace --stats -- python
tools/gnn_bench.py` and read k_cgen_im2col* / k_gnn_col2im in the kernel statistics.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cgs_vmc_amd import _hip  # noqa: E402
from oracle import vmc_oracle as vo  # noqa: E402
from tests import gnn_oracle as go  # noqa: E402

_GENERAL_IM2COL = {'CGS_VMC_CONV_GENERAL': '1', 'CGS_VMC_CONV_BAND': '0', 'CGS_VMC_CONV_GENERAL_IMPLICIT': '0',
                   'CGS_VMC_CONV_PATCH': '0'}
_KNOBS = tuple(_GENERAL_IM2COL)


def _time_step(eng, n_sites, bonds, theta, cfg, reps, warmup=2):
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, -1.0, 1.0)

  def step():
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.mc_steps(n_sites, want_accepted=False)

  for _ in range(warmup):
    step()
  eng.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    step()
  eng.synchronize()
  return (time.perf_counter() - t0) / reps * 1e3


def _case(name, n_sites, L, f, bonds, chains, reps, env=None, **kw):
  from cgs_vmc_amd.engine import VmcEngine
  saved = {k: os.environ.pop(k, None) for k in _KNOBS}
  os.environ.update(env or {})
  try:
    eng = VmcEngine(n_sites, chains, L, f, seed=2024, **kw)
    rng = np.random.default_rng(0)
    if kw['ansatz'] == 'gnn':
      theta = go.gnn_init_params(kw['adjacency'].shape[1], f, L, rng, noise=0.01)
    else:
      theta = vo.conv_init_params('conv_2d', (f, kw['kernel_size'], kw['size_x'], kw['size_y']), L, rng)
    cfg = vo.random_configurations(n_sites, chains, np.random.RandomState(1))
    ms = _time_step(eng, n_sites, bonds, theta, cfg, reps)
    line = dict(case=name, sites=n_sites, chains=chains, layers=L, filters=f, kernel_path=eng.kernel_path(),
                ms_per_step=round(ms, 3), us_per_mc_step=round(1e3 * ms / n_sites, 2))
    eng.close()
  finally:
    for k in _KNOBS:
      os.environ.pop(k, None)
      if saved[k] is not None:
        os.environ[k] = saved[k]
  print(json.dumps(line), flush=True)
  return line


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--chains', type=int, default=1024)
  ap.add_argument('--reps', type=int, default=5)
  a = ap.parse_args(argv)
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('gnn_bench: no GPU')
  tri = go.triangular_adjacency(12, 12)
  tri_bonds = go.triangular_bonds(12, 12)
  for f in (16, 64):
    _case('gnn triangular 12x12 k=7 3x%d' % f, 144, 3, f, tri_bonds, a.chains, a.reps, ansatz='gnn', adjacency=tri)
  sq_bonds = vo.torus_bonds(10, 10)
  _case('gnn square 10x10 5-point 3x16', 100, 3, 16, sq_bonds, a.chains, a.reps, ansatz='gnn',
        adjacency=go.square_5point_adjacency(10, 10))
  # the 3 x 3 stencil as a graph beside conv_2d K = 3 on the same 10 x 10 torus
  _case('gnn square 10x10 3x3 stencil 3x16', 100, 3, 16, sq_bonds, a.chains, a.reps, ansatz='gnn',
        adjacency=go.stencil_adjacency(10, 10, 3))
  conv = dict(ansatz='conv_2d', kernel_size=3, size_x=10, size_y=10)
  _case('conv_2d 10x10 K=3 3x16 general im2col', 100, 3, 16, sq_bonds, a.chains, a.reps, env=_GENERAL_IM2COL, **conv)
  _case('conv_2d 10x10 K=3 3x16 default path', 100, 3, 16, sq_bonds, a.chains, a.reps, **conv)


if __name__ == '__main__':
  main()

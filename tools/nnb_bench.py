#!/usr/bin/env python3
"""Time of one training inner-loop step of the fully_connected_nnb ansatz -- accumulate (EnergyGradient) + one sweep
(num_sites mc_steps), the body of run_optimization_epoch (training.py:608-617) -- with the sampler, local-energy and
gradient shares from vmc_timing ("sweep", "tail_eloc", "grad"); for scale, the same step of pbdg and of fully_connected
with the same trunk on the same lattice and batch.

  python tools/nnb_bench.py [--reps 3] [--out FILE]

Host clock around synchronised work after a warm-up, then a second pass with per-region HIP events (which drain the
pipeline between kernels: the split, not the total, is what that pass is for).  Needs a GPU.  One JSON line per case:
the 6 x 6 (L = 2, H = 64) and 10 x 10 (L = 3, H = 256) square tori at 4,096 chains.
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
from tests import nnb_oracle as no  # noqa: E402


def _case(name, ansatz, n_sites, bonds, chains, layers, units, reps, warmup=1):
  from cgs_vmc_amd.engine import VmcEngine
  if ansatz == 'pbdg':
    eng = VmcEngine(n_sites, chains, 1, 1, ansatz='pbdg', seed=2024)
    lim = np.sqrt(3.0 / n_sites)
    eng.set_params(np.random.default_rng(0).uniform(-lim, lim, n_sites * n_sites).astype(np.float32))
  elif ansatz == 'fully_connected':
    eng = VmcEngine(n_sites, chains, layers, units, seed=2024)
    eng.set_params(vo.init_params(n_sites, units, layers, np.random.default_rng(0)))
  else:
    eng = VmcEngine(n_sites, chains, layers, units, ansatz='fully_connected_nnb', seed=2024)
    eng.set_params(no.default_theta(n_sites, layers, units, 0))
  eng.set_configs(vo.random_configurations(n_sites, chains, np.random.RandomState(1)))
  eng.set_bonds(bonds, 1.0, 1.0)

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
  ms = (time.perf_counter() - t0) / reps * 1e3
  eng.timing_enable(True)
  eng.timing_reset()
  for _ in range(reps):
    step()
  eng.synchronize()
  split = {k: round(eng.timing_get(k)[0] / reps, 3) for k in ('sweep', 'tail_eloc', 'grad', 'bond_list', 'eloc_reduce')}
  line = dict(case=name, sites=n_sites, chains=chains, kernel_path=eng.kernel_path(), ms_per_step=round(ms, 3),
              us_per_mc_step=round(1e3 * split['sweep'] / n_sites, 2), ms_split=split)
  eng.close()
  print(json.dumps(line), flush=True)
  return line


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--out', default=None, help='also write the lines to this file')
  a = ap.parse_args(argv)
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('nnb_bench: no GPU')
  lines = [
      _case('nnb square 6x6', 'fully_connected_nnb', 36, vo.torus_bonds(6, 6), 4096, 2, 64, a.reps),
      _case('nnb square 10x10', 'fully_connected_nnb', 100, vo.torus_bonds(10, 10), 4096, 3, 256, a.reps),
      _case('pbdg square 10x10', 'pbdg', 100, vo.torus_bonds(10, 10), 4096, 1, 1, a.reps),
      _case('fully_connected square 10x10', 'fully_connected', 100, vo.torus_bonds(10, 10), 4096, 3, 256, a.reps),
  ]
  if a.out:
    with open(a.out, 'w') as f:
      for line in lines:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
  main()

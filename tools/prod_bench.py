#!/usr/bin/env python3
"""Time of one training inner-loop step of the prod composite pbdg x fully_connected -- accumulate (EnergyGradient) + one
sweep (num_sites mc_steps), the body of run_optimization_epoch (training.py:608-617) -- beside the same step of each
factor alone at the same shape.

  python tools/prod_bench.py [--reps 5] [--out profiles/prod_bench.jsonl]

Host clock around synchronised work after a warm-up.  No step time is promised for the composite: it evaluates two
full forwards per Metropolis step (several launches) where the factors alone run incremental samplers in one persistent
launch; the lines record by how much it is slower.  Needs a GPU.  One JSON line per shape: 6 x 6 and 10 x 10 square tori
at 4,096 chains, the dense factor with 2 layers of 64 units.
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

H, L = 64, 2


def _time_step(eng, n_sites, reps, warmup=2):
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


def _case(name, n_sites, bonds, chains, reps):
  from cgs_vmc_amd.engine import VmcEngine
  lim = np.sqrt(3.0 / n_sites)
  th_p = np.random.default_rng(0).uniform(-lim, lim, n_sites * n_sites).astype(np.float32)
  th_f = vo.init_params(n_sites, H, L, np.random.default_rng(1))
  cfg = vo.random_configurations(n_sites, chains, np.random.RandomState(1))
  specs = dict(
      pbdg=dict(ansatz='pbdg', num_layers=1, layer_size=1),
      fully_connected=dict(ansatz='fully_connected', num_layers=L, layer_size=H))
  ms = {}
  for key, theta in (('pbdg', th_p), ('fully_connected', th_f), ('prod', np.concatenate([th_p, th_f]))):
    if key == 'prod':
      eng = VmcEngine(n_sites, chains, 0, 0, ansatz='prod', seed=2024, children=[specs['pbdg'], specs['fully_connected']])
    else:
      eng = VmcEngine(n_sites, chains, seed=2024, **specs[key])
    eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, 1.0, 1.0)
    ms[key] = round(_time_step(eng, n_sites, reps), 3)
    eng.close()
  line = dict(case=name, sites=n_sites, chains=chains, dense_units=H, dense_layers=L, ms_per_step=ms,
              prod_over_sum_of_factors=round(ms['prod'] / (ms['pbdg'] + ms['fully_connected']), 2),
              us_per_prod_mc_step_upper=round(1e3 * ms['prod'] / n_sites, 2))
  print(json.dumps(line), flush=True)
  return line


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=None, help='also write the lines to this file')
  a = ap.parse_args(argv)
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('prod_bench: no GPU')
  lines = [
      _case('prod(pbdg, fully_connected) square 6x6', 36, vo.torus_bonds(6, 6), 4096, a.reps),
      _case('prod(pbdg, fully_connected) square 10x10', 100, vo.torus_bonds(10, 10), 4096, a.reps),
  ]
  if a.out:
    with open(a.out, 'w') as f:
      for line in lines:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
  main()

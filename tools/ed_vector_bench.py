#!/usr/bin/env python3
"""Kernel times of the ed_vector ansatz at three vector sizes: N = 16 (12,870 entries, 51 KB), N = 24 (2,704,156
entries, 10.8 MB) and N = 28 (40,116,600 entries, 160 MB), positive random vectors on a periodic chain.

  python tools/ed_vector_bench.py [--chains 65536] [--reps 5] [--out FILE]

Per size one JSON line: the time of one mc_step of all chains (a persistent launch of 4 N steps, vmc_timing "sweep"),
sweeps (N mc_steps of every chain) per second, local-energy evaluations (chains) per second ("tail_eloc" +
"bond_list" + "eloc_reduce") and the time of the gradient scatter ("grad": keys, radix sort, segmented sums), plus
gathers per second of the sampler (one dependent vector gather per chain and step).  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cgs_vmc_amd import _hip, lattice  # noqa: E402
from oracle import vmc_oracle as vo  # noqa: E402
from tools import make_ed_vector as mk  # noqa: E402


def _case(n_sites, chains, reps):
  from cgs_vmc_amd.engine import VmcEngine
  top, bot, length = mk.lin_tables(n_sites)
  eng = VmcEngine(n_sites, chains, 1, length, ansatz='ed_vector', seed=2024,
                  lin_tables=(top.astype(np.int32), bot.astype(np.int32)))
  eng.set_params(np.random.default_rng(0).uniform(0.5, 1.5, length).astype(np.float32))
  eng.set_configs(vo.random_configurations(n_sites, chains, np.random.RandomState(1)))
  eng.set_bonds(lattice.chain_bonds(n_sites), 1.0, 1.0)
  steps = 4 * n_sites

  def step():
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.mc_steps(steps, want_accepted=False)

  for _ in range(2):
    step()
  eng.synchronize()
  eng.timing_enable(True)
  eng.timing_reset()
  for _ in range(reps):
    step()
  eng.synchronize()
  ms = {k: eng.timing_get(k)[0] / reps for k in ('sweep', 'tail_eloc', 'bond_list', 'eloc_reduce', 'grad')}
  eloc_ms = ms['tail_eloc'] + ms['bond_list'] + ms['eloc_reduce']
  us_step = 1e3 * ms['sweep'] / steps
  line = dict(sites=n_sites, entries=length, vector_mb=round(4e-6 * length, 2), chains=chains,
              kernel_path=eng.kernel_path(), us_per_mc_step=round(us_step, 3),
              sweeps_per_s=round(1e6 / (us_step * n_sites), 1), gathers_per_s=round(chains / (us_step * 1e-6), 0),
              eloc_ms=round(eloc_ms, 4), eloc_evals_per_s=round(chains / (eloc_ms * 1e-3), 0),
              scatter_ms=round(ms['grad'], 4),
              ms_split={k: round(v, 4) for k, v in ms.items()})
  eng.close()
  print(json.dumps(line), flush=True)
  return line


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--chains', type=int, default=65536)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--sites', type=int, nargs='+', default=[16, 24, 28])
  ap.add_argument('--out', default='')
  args = ap.parse_args()
  lines = [_case(n, args.chains, args.reps) for n in args.sites]
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      for line in lines:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
  main()

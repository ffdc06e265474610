#!/usr/bin/env python3
"""One all-pairs spin-correlation measurement next to one local-energy call at BASELINE config 3's shape: the 10 x 10
Heisenberg torus (200 bonds), fully_connected 3 x 256, 4,096 chains; 4,950 pairs against 200 bonds.

  python tools/corr_bench.py [--chains 4096] [--reps 5] [--pairs_per_pass 0] [--out FILE]

One JSON line: wall time of engine.pair_correlations (host call, read-back included) and of engine.local_energy, the
vmc_timing regions of both ("bond_list", "tail_eloc", "corr_fold", "eloc_reduce"), connected rows per second of either.
Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cgs_vmc_amd import lattice  # noqa: E402
from oracle import vmc_oracle as vo  # noqa: E402

REGIONS = ('bond_list', 'tail_eloc', 'corr_fold', 'eloc_reduce')


def _timed(eng, fn, reps):
  for _ in range(2):
    fn()
  eng.synchronize()
  eng.timing_enable(True)
  eng.timing_reset()
  t0 = time.perf_counter()
  for _ in range(reps):
    fn()
  eng.synchronize()
  wall = (time.perf_counter() - t0) / reps
  ms = {k: round(eng.timing_get(k)[0] / reps, 4) for k in REGIONS}
  eng.timing_enable(False)
  return 1e3 * wall, ms


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--chains', type=int, default=4096)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--pairs_per_pass', type=int, default=0)
  ap.add_argument('--out', default='')
  args = ap.parse_args(argv)
  from cgs_vmc_amd.engine import VmcEngine
  n, h, layers = 100, 256, 3
  bonds = lattice.torus_bonds(10, 10)
  pairs = lattice.all_pairs(n)
  eng = VmcEngine(n, args.chains, layers, h, seed=2024)
  eng.set_params(vo.init_params(n, h, layers, np.random.default_rng(0)))
  eng.set_configs(vo.random_configurations(n, args.chains, np.random.RandomState(1)))
  eng.set_bonds(bonds, 1.0, 1.0)
  eng.mc_steps(4 * n, want_accepted=False)
  eloc_ms, eloc_regions = _timed(eng, lambda: eng.local_energy(want_eloc=False), args.reps)
  eloc_rows = eng.last_connected_rows()
  cfg = eng.get_configs()
  corr_rows = int((cfg[:, pairs[:, 0]] != cfg[:, pairs[:, 1]]).sum())
  corr_ms, corr_regions = _timed(eng, lambda: eng.pair_correlations(pairs, pairs_per_pass=args.pairs_per_pass), args.reps)
  line = dict(sites=n, chains=args.chains, network='fully_connected 3x256', bonds=len(bonds), pairs=len(pairs),
              pairs_per_pass=args.pairs_per_pass, kernel_path=eng.kernel_path(),
              local_energy_ms=round(eloc_ms, 4), local_energy_rows=eloc_rows,
              local_energy_rows_per_s=round(eloc_rows / (eloc_ms * 1e-3), 0), local_energy_regions_ms=eloc_regions,
              correlations_ms=round(corr_ms, 4), correlation_rows=corr_rows,
              correlation_rows_per_s=round(corr_rows / (corr_ms * 1e-3), 0), correlation_regions_ms=corr_regions,
              ratio_ms=round(corr_ms / eloc_ms, 2), ratio_rows=round(corr_rows / max(eloc_rows, 1), 2))
  eng.close()
  text = json.dumps(line)
  print(text, flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
      f.write(text + '\n')
  return line


if __name__ == '__main__':
  main()

#!/usr/bin/env python3
"""One Renyi-2 swap measurement over the 50 block regions next to one local-energy call at BASELINE config 3's shape: the
10 x 10 Heisenberg torus (200 bonds), fully_connected 3 x 256, 4,096 chains (2,048 replica pairs).

  python tools/renyi_bench.py [--chains 4096] [--reps 5] [--regions_per_pass 0] [--out profiles/renyi_bench.jsonl]

One JSON line, appended to --out: wall time of engine.renyi2_swap (host call, read-back included) and of
engine.local_energy, the vmc_timing regions of both ("renyi_rows", "renyi_forward", "renyi_fold"; "bond_list",
"tail_eloc", "eloc_reduce"), rows per second of either -- the measurement's rows are FULL forwards of swapped
configurations (regions x chains of them, the unswapped rows of non-matching pairs included), the local energy's are
rank-2 updates of the cached first layer.  Needs a GPU."""
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

REGIONS = ('renyi_rows', 'renyi_forward', 'renyi_fold', 'bond_list', 'tail_eloc', 'eloc_reduce')


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
  return 1e3 * wall, {k: v for k, v in ms.items() if v > 0}


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--chains', type=int, default=4096)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--regions_per_pass', type=int, default=0)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'renyi_bench.jsonl'))
  args = ap.parse_args(argv)
  from cgs_vmc_amd.engine import VmcEngine
  n, h, layers = 100, 256, 3
  bonds = lattice.torus_bonds(10, 10)
  masks = lattice.region_masks(lattice.block_regions(n), n)
  eng = VmcEngine(n, args.chains, layers, h, seed=2024)
  eng.set_params(vo.init_params(n, h, layers, np.random.default_rng(0)))
  eng.set_configs(vo.random_configurations(n, args.chains, np.random.RandomState(1)))
  eng.set_bonds(bonds, 1.0, 1.0)
  eng.mc_steps(4 * n, want_accepted=False)
  eloc_ms, eloc_regions = _timed(eng, lambda: eng.local_energy(want_eloc=False), args.reps)
  eloc_rows = eng.last_connected_rows()
  swap, match = eng.renyi2_swap(masks, regions_per_pass=args.regions_per_pass)
  rows = len(masks) * args.chains
  renyi_ms, renyi_regions = _timed(eng, lambda: eng.renyi2_swap(masks, regions_per_pass=args.regions_per_pass), args.reps)
  line = dict(sites=n, chains=args.chains, network='fully_connected 3x256', bonds=len(bonds), regions=len(masks),
              regions_per_pass=args.regions_per_pass, kernel_path=eng.kernel_path(),
              local_energy_ms=round(eloc_ms, 4), local_energy_rows=eloc_rows,
              local_energy_rows_per_s=round(eloc_rows / (eloc_ms * 1e-3), 0), local_energy_regions_ms=eloc_regions,
              renyi_ms=round(renyi_ms, 4), renyi_rows=rows, renyi_swapped_rows=int(2 * match.sum()),
              renyi_rows_per_s=round(rows / (renyi_ms * 1e-3), 0), renyi_regions_ms=renyi_regions,
              ratio_ms=round(renyi_ms / eloc_ms, 2), ratio_rows=round(rows / max(eloc_rows, 1), 2),
              match_fraction_min=round(float(match.min() / (args.chains // 2)), 4))
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

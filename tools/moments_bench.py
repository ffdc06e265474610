#!/usr/bin/env python3
"""One Lanczos-step measurement (engine.energy_moments: the local values of H and H^2 per chain) next to one local-energy
call at BASELINE config 3's shape: the 10 x 10 Heisenberg torus (200 bonds), fully_connected 3 x 256, 4,096 chains.

  python tools/moments_bench.py [--chains 4096] [--reps 3] [--rows_per_pass 0] [--out profiles/moments_bench.jsonl]

One JSON line, appended to --out: wall time of engine.energy_moments (host call, the two row-count read-backs and the
read-back of the sums included) and of engine.local_energy, n_rows2 -- the length of the compacted list of doubly exchanged
configurations, each a FULL forward -- next to the n_bonds^2 x chains rows the all-pairs dimer route would forward, the
passes the list took, the vmc_timing regions "mom_eloc" (the local-energy call inside), "mom_list" (count, prefix and the
passes' descriptors), "mom_rows", "mom_forward", "mom_fold", and the rows per second.  Needs a GPU."""
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

REGIONS = ('mom_eloc', 'mom_list', 'mom_rows', 'mom_forward', 'mom_fold', 'bond_list', 'tail_eloc', 'eloc_reduce')


def _timed(eng, fn, reps, warm):
  for _ in range(warm):
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
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--rows_per_pass', type=int, default=0)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moments_bench.jsonl'))
  args = ap.parse_args(argv)
  from cgs_vmc_amd.engine import VmcEngine
  n, h, layers = 100, 256, 3
  bonds = lattice.torus_bonds(10, 10)
  eng = VmcEngine(n, args.chains, layers, h, seed=2024)
  eng.set_params(vo.init_params(n, h, layers, np.random.default_rng(0)))
  eng.set_configs(vo.random_configurations(n, args.chains, np.random.RandomState(1)))
  eng.set_bonds(bonds, 1.0, 1.0)
  eng.mc_steps(4 * n, want_accepted=False)
  eloc_ms, eloc_regions = _timed(eng, lambda: eng.local_energy(want_eloc=False), args.reps, 2)
  eloc_rows = eng.last_connected_rows()
  out = eng.energy_moments(rows_per_pass=args.rows_per_pass)          # (also the warm-up: the buffers grow here)
  mom_ms, mom_regions = _timed(eng, lambda: eng.energy_moments(rows_per_pass=args.rows_per_pass), args.reps, 0)
  rows = out['n_rows2']
  alive = max(out['n_alive'], 1)
  line = dict(sites=n, chains=args.chains, network='fully_connected 3x256', bonds=len(bonds),
              rows_per_pass=args.rows_per_pass, kernel_path=eng.kernel_path(),
              local_energy_ms=round(eloc_ms, 4), local_energy_rows=eloc_rows, local_energy_regions_ms=eloc_regions,
              moments_ms=round(mom_ms, 4), n_rows2=rows, n_rows2_per_chain=round(rows / args.chains, 1),
              all_pairs_rows=len(bonds) ** 2 * args.chains, moments_rows_per_s=round(rows / (mom_ms * 1e-3), 0),
              moments_regions_ms=mom_regions, ratio_to_local_energy=round(mom_ms / eloc_ms, 2),
              h1=out['e_sum'] / alive, h2=out['e2_sum'] / alive, h2_check=out['g_sum'] / alive, h3=out['eg_sum'] / alive,
              h4=out['g2_sum'] / alive, finite=bool(all(np.isfinite(out[k]) for k in ('e_sum', 'e2_sum', 'g_sum', 'eg_sum', 'g2_sum'))))
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

#!/usr/bin/env python3
"""One dimer-dimer measurement -- one reference bond against all 200 bonds -- next to one local-energy call at BASELINE
config 3's shape: the 10 x 10 Heisenberg torus (200 bonds), fully_connected 3 x 256, 4,096 chains.

  python tools/dimer_bench.py [--chains 4096] [--reps 5] [--reference_bond 0] [--pairs_per_pass 0] [--out profiles/dimer_bench.jsonl]

One JSON line, appended to --out: wall time of engine.dimer_correlations (host call, read-back included) and of
engine.local_energy, the vmc_timing regions of both ("dimer_rows", "dimer_forward", "dimer_fold"; "bond_list",
"tail_eloc", "eloc_reduce"), rows per second of either and the ratio of the two times -- the measurement's rows are FULL
forwards of exchanged configurations ((bonds + pairs) x chains of them, the unexchanged rows of parallel bonds
included), the local energy's are rank-2 updates of the cached first layer.  No target is set: the line records what
was measured.  Needs a GPU."""
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

REGIONS = ('dimer_rows', 'dimer_forward', 'dimer_fold', 'bond_list', 'tail_eloc', 'eloc_reduce')


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
  ap.add_argument('--reference_bond', type=int, default=0)
  ap.add_argument('--pairs_per_pass', type=int, default=0)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dimer_bench.jsonl'))
  args = ap.parse_args(argv)
  from cgs_vmc_amd.engine import VmcEngine
  n, h, layers = 100, 256, 3
  bonds = lattice.torus_bonds(10, 10)
  pairs = [(args.reference_bond, b) for b in range(len(bonds))]
  eng = VmcEngine(n, args.chains, layers, h, seed=2024)
  eng.set_params(vo.init_params(n, h, layers, np.random.default_rng(0)))
  eng.set_configs(vo.random_configurations(n, args.chains, np.random.RandomState(1)))
  eng.set_bonds(bonds, 1.0, 1.0)
  eng.mc_steps(4 * n, want_accepted=False)
  eloc_ms, eloc_regions = _timed(eng, lambda: eng.local_energy(want_eloc=False), args.reps)
  eloc_rows = eng.last_connected_rows()
  measure = lambda: eng.dimer_correlations(bonds, pairs, pairs_per_pass=args.pairs_per_pass)
  bond_sum, dd_sum = measure()
  rows = (len(bonds) + len(pairs)) * args.chains
  dimer_ms, dimer_regions = _timed(eng, measure, args.reps)
  line = dict(sites=n, chains=args.chains, network='fully_connected 3x256', bonds=len(bonds), pairs=len(pairs),
              reference_bond=args.reference_bond, pairs_per_pass=args.pairs_per_pass, kernel_path=eng.kernel_path(),
              local_energy_ms=round(eloc_ms, 4), local_energy_rows=eloc_rows,
              local_energy_rows_per_s=round(eloc_rows / (eloc_ms * 1e-3), 0), local_energy_regions_ms=eloc_regions,
              dimer_ms=round(dimer_ms, 4), dimer_rows=rows, dimer_rows_per_s=round(rows / (dimer_ms * 1e-3), 0),
              dimer_regions_ms=dimer_regions, ratio_ms=round(dimer_ms / eloc_ms, 2),
              ratio_rows=round(rows / max(eloc_rows, 1), 2),
              bond_mean=round(float(bond_sum.mean() / args.chains), 6),
              dd_self=round(float(dd_sum[args.reference_bond] / args.chains), 6))
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

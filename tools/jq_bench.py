#!/usr/bin/env python3
"""One accumulate + sweep with and without the four-spin (J-Q) terms at BASELINE config 3's shape: the 10 x 10 torus
(200 bonds, the 200 plaquette terms of lattice.jq_torus_terms), fully_connected 3 x 256, 4,096 chains.

  python tools/jq_bench.py [--chains 4096] [--reps 5] [--sweep_steps 100] [--rows_per_pass 0] [--out profiles/jq_bench.jsonl]

One JSON line, appended to --out: wall time of one step -- engine.accumulate(ENERGY_GRADIENT) followed by
engine.mc_steps(sweep_steps) -- on the Heisenberg Hamiltonian alone and with the terms set, the vmc_timing regions of the
term pass ("fs_list", "fs_rows", "fs_forward", "fs_fold") and of the Heisenberg rows ("bond_list", "tail_eloc",
"eloc_reduce"), the lengths of the term list and its rows per second.  The term rows are FULL forwards of exchanged
configurations (one per antiparallel pair and one per active term of every chain); the Heisenberg rows are rank-2
updates of the cached first layer.  No target is set: the line records what was measured.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cgs_vmc_amd import _hip  # noqa: E402
from cgs_vmc_amd import lattice  # noqa: E402
from oracle import vmc_oracle as vo  # noqa: E402

REGIONS = ('fs_list', 'fs_rows', 'fs_forward', 'fs_fold', 'bond_list', 'tail_eloc', 'eloc_reduce', 'sweep')


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
  ap.add_argument('--sweep_steps', type=int, default=100)
  ap.add_argument('--rows_per_pass', type=int, default=0)
  ap.add_argument('--q', type=float, default=1.0)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jq_bench.jsonl'))
  args = ap.parse_args(argv)
  from cgs_vmc_amd.engine import VmcEngine
  n, h, layers = 100, 256, 3
  bonds = lattice.torus_bonds(10, 10)
  terms = lattice.jq_torus_terms(10, 10)
  eng = VmcEngine(n, args.chains, layers, h, seed=2024)
  eng.set_params(vo.init_params(n, h, layers, np.random.default_rng(0)))
  eng.set_configs(vo.random_configurations(n, args.chains, np.random.RandomState(1)))
  eng.set_bonds(bonds, -1.0, 1.0)
  eng.mc_steps(4 * n, want_accepted=False)

  def step():
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.mc_steps(args.sweep_steps, want_accepted=False)
  eng.reset_accumulators()
  plain_ms, plain_regions = _timed(eng, step, args.reps)
  eng.set_four_spin_terms(terms, args.q, -1, rows_per_pass=args.rows_per_pass)
  eng.reset_accumulators()
  jq_ms, jq_regions = _timed(eng, step, args.reps)
  single, double = eng.last_four_spin_rows()
  term_ms = sum(jq_regions.get(k, 0.0) for k in REGIONS[:4])
  line = dict(sites=n, chains=args.chains, network='fully_connected 3x256', bonds=len(bonds), terms=len(terms), q=args.q,
              sweep_steps=args.sweep_steps, rows_per_pass=args.rows_per_pass, kernel_path=eng.kernel_path(),
              step_ms=round(plain_ms, 4), step_regions_ms=plain_regions,
              step_with_terms_ms=round(jq_ms, 4), step_with_terms_regions_ms=jq_regions,
              single_rows=single, double_rows=double, term_pass_ms=round(term_ms, 4),
              term_rows_per_s=round((single + double) / max(term_ms * 1e-3, 1e-12), 0),
              ratio_ms=round(jq_ms / plain_ms, 2), mean_energy=round(eng.mean_energy(), 6))
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

#!/usr/bin/env python3
"""One projected-energy measurement -- the 100 translations with and without the global spin flip, 200 ops, and all 104
sectors of lattice.sector_characters(10, 10, True) -- next to one symmetry measurement of the same ops (tools/symm_bench.py's
line) and one local-energy call at BASELINE config 3's shape: the 10 x 10 Heisenberg torus (200 bonds), fully_connected
3 x 256, 4,096 chains.

  python tools/proj_bench.py [--chains 4096] [--reps 5] [--ops_per_pass 0] [--out profiles/proj_bench.jsonl]

One JSON line, appended to --out: wall time of engine.projected_energy (host call, both validations, uploads and
read-back included), of engine.symmetry_expectations and of engine.local_energy, the vmc_timing regions of each -- for
the projection "proj_eloc" (the local-energy call inside it), "proj_rows", "proj_forward", "proj_accum", "proj_fold" --
and the rows per second.  The measurement's rows are FULL forwards of permuted configurations (ops x chains of them);
the accumulation is ops x sectors x chains fp64 fused multiply-adds.  Needs a GPU."""
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

REGIONS = ('proj_eloc', 'proj_rows', 'proj_forward', 'proj_accum', 'proj_fold', 'symm_rows', 'symm_forward', 'symm_fold',
           'bond_list', 'tail_eloc', 'eloc_reduce')


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
  ap.add_argument('--ops_per_pass', type=int, default=0)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'proj_bench.jsonl'))
  args = ap.parse_args(argv)
  from cgs_vmc_amd.engine import VmcEngine
  n, h, layers = 100, 256, 3
  bonds = lattice.torus_bonds(10, 10)
  t = lattice.translations(10, 10)
  perms = np.concatenate([t, t])
  flips = np.repeat([0, 1], n).astype(np.uint8)
  labels, chi = lattice.sector_characters(10, 10, True)
  eng = VmcEngine(n, args.chains, layers, h, seed=2024)
  eng.set_params(vo.init_params(n, h, layers, np.random.default_rng(0)))
  eng.set_configs(vo.random_configurations(n, args.chains, np.random.RandomState(1)))
  eng.set_bonds(bonds, 1.0, 1.0)
  eng.mc_steps(4 * n, want_accepted=False)
  eloc_ms, eloc_regions = _timed(eng, lambda: eng.local_energy(want_eloc=False), args.reps)
  eloc_rows = eng.last_connected_rows()
  symm_ms, symm_regions = _timed(eng, lambda: eng.symmetry_expectations(perms, flips, ops_per_pass=args.ops_per_pass), args.reps)
  out = eng.projected_energy(perms, flips, chi, ops_per_pass=args.ops_per_pass)
  rows = len(perms) * args.chains
  proj_ms, proj_regions = _timed(eng, lambda: eng.projected_energy(perms, flips, chi, ops_per_pass=args.ops_per_pass), args.reps)
  line = dict(sites=n, chains=args.chains, network='fully_connected 3x256', bonds=len(bonds), ops=len(perms),
              sectors=len(labels), ops_per_pass=args.ops_per_pass, kernel_path=eng.kernel_path(),
              local_energy_ms=round(eloc_ms, 4), local_energy_rows=eloc_rows, local_energy_regions_ms=eloc_regions,
              symm_ms=round(symm_ms, 4), symm_regions_ms=symm_regions,
              proj_ms=round(proj_ms, 4), proj_rows=rows, proj_rows_per_s=round(rows / (proj_ms * 1e-3), 0),
              proj_fmas=len(perms) * len(labels) * args.chains, proj_regions_ms=proj_regions,
              ratio_to_local_energy=round(proj_ms / eloc_ms, 2), ratio_to_symm=round(proj_ms / symm_ms, 2),
              weight_sum_per_chain=float(out['w_sum'].sum() / max(out['n_alive'], 1)),
              completeness=float(out['we_sum'].sum() - out['e_sum']),
              finite=bool(np.isfinite(out['w_sum']).all() and np.isfinite(out['we_sum']).all()))
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

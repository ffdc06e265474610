#!/usr/bin/env python3
"""The penalised accumulate (vmc_accumulate mode PENALIZED_ENERGY: E + lambda F against the frozen parameter set) next to
the plain energy-gradient accumulate, and vmc_overlap alone, at BASELINE config 3's shape: the 10 x 10 Heisenberg torus,
fully_connected 3 x 256, 4,096 chains.

  python tools/overlap_bench.py [--chains 4096] [--reps 200] [--rounds 5] [--out profiles/overlap_bench.jsonl]

A training step is [accumulate, one sweep of n_sites mc_steps]: after the sweep the chains are new, so the frozen set's
amplitude cache is rebuilt by every mode-2 accumulate, as in an epoch.  Per round the script times `reps` such steps with
mode 0, then with mode 2 (a host clock around work that ends in a synchronise; both warmed up first), and `reps` calls of
[vmc_overlap, one sweep] less the sweeps alone; the rounds alternate the two modes so that drift of the shared machine
hits both.  One JSON line, appended to --out: the medians over the rounds in ms per step, the ratio mode 2 / mode 0 per
round (median, min, max), vmc_overlap's time, and the vmc_timing regions of one mode-2 step.  Mode 0 runs the kernels
it ran before mode 2 existed (tests/test_gpu_path_bits.py pins its bits).  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cgs_vmc_amd import _hip, lattice  # noqa: E402
from oracle import vmc_oracle as vo  # noqa: E402

REGIONS = ('tail_eloc', 'eloc_reduce', 'z1', 'tail_amp', 'overlap_fold', 'overlap_weights', 'grad', 'sweep')


def _steps(eng, fn, n, reps):
  """ms per [fn, sweep] over `reps` of them."""
  eng.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    fn()
    eng.mc_steps(n, want_accepted=False)
  eng.synchronize()
  return 1e3 * (time.perf_counter() - t0) / reps


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--chains', type=int, default=4096)
  ap.add_argument('--reps', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--penalty', type=float, default=1.0)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'overlap_bench.jsonl'))
  args = ap.parse_args(argv)
  from cgs_vmc_amd.engine import VmcEngine
  n, h, layers = 100, 256, 3
  eng = VmcEngine(n, args.chains, layers, h, seed=2024)
  theta = vo.init_params(n, h, layers, np.random.default_rng(0))
  eng.set_params(theta)
  eng.set_params(theta + (0.02 * np.random.default_rng(8).standard_normal(theta.size)).astype(np.float32), _hip.VMC_OMEGA)
  eng.set_configs(vo.random_configurations(n, args.chains, np.random.RandomState(1)))
  eng.set_bonds(lattice.torus_bonds(10, 10), 1.0, 1.0)
  eng.mc_steps(4 * n, want_accepted=False)
  eng.reset_accumulators()
  plain = lambda: eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  penalised = lambda: eng.accumulate(_hip.VMC_MODE_PENALIZED_ENERGY, args.penalty)
  for fn in (plain, penalised, eng.overlap, lambda: None):          # warm-up of every shape the windows use
    _steps(eng, fn, n, 3)
  rows = []
  for _ in range(args.rounds):
    eng.reset_accumulators()
    m0 = _steps(eng, plain, n, args.reps)
    eng.reset_accumulators()
    m2 = _steps(eng, penalised, n, args.reps)
    ov = _steps(eng, eng.overlap, n, args.reps)
    sw = _steps(eng, lambda: None, n, args.reps)
    rows.append((m0, m2, ov - sw, sw))
  rows = np.array(rows)
  ratios = rows[:, 1] / rows[:, 0]
  eng.timing_enable(True); eng.timing_reset()
  _steps(eng, penalised, n, args.reps)
  regions = {k: round(eng.timing_get(k)[0] / args.reps, 4) for k in REGIONS}
  eng.timing_enable(False)
  fid = eng.overlap()
  line = dict(sites=n, chains=args.chains, network='fully_connected 3x256', kernel_path=eng.kernel_path(), reps=args.reps,
              rounds=args.rounds, step_mode0_ms=round(float(np.median(rows[:, 0])), 4),
              step_mode2_ms=round(float(np.median(rows[:, 1])), 4), sweep_ms=round(float(np.median(rows[:, 3])), 4),
              overlap_ms=round(float(np.median(rows[:, 2])), 4), ratio_mode2_to_mode0=round(float(np.median(ratios)), 4),
              ratio_min=round(float(ratios.min()), 4), ratio_max=round(float(ratios.max()), 4),
              mode2_regions_ms={k: v for k, v in regions.items() if v > 0},
              fidelity=fid['s1'] ** 2 / (fid['alive'] * fid['s2']), log_scale=fid['log_scale'])
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

#!/usr/bin/env python3
"""Time of one training inner-loop step of the symmetrized ansatz -- accumulate (EnergyGradient) + one sweep (num_sites
mc_steps) -- at the shape of config 3: the 10 x 10 torus, a fully_connected base of 3 x 256 units, the 100 translations in
the trivial sector, a symmetrized batch of 64 chains and therefore a base of 6,400 rows.

  python tools/symmetrized_bench.py [--reps 5] [--out profiles/symmetrized_bench.jsonl]

Host clock around synchronised work after a warm-up, and the library's own regions ("sweep", "symz_rows", "symz_fold",
"eloc_fold", "grad") per step.  Beside them, on the device clock too: the BASE ctx's own regions during the same steps
(its forwards "z1" + "tail_amp", its row list, rows and reductions, its gradient path) and, on a plain ctx of the base's
shape, vmc_amplitude of its own 6,400 chains (configs == NULL, the cache dropped before each call: one full forward, no
host rows) times the number of full forwards a step makes (one per mc_step, one for the accumulate).  The share of a step
that is not the base's own kernels is 1 - (the base's regions) / (the step).  No threshold: the feature is judged on
correctness; the line records what it costs.  Appends one JSON line.  Needs a GPU.
"""
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

SX = SY = 10
H, L, B = 256, 3, 64
REGIONS = ('sweep', 'symz_rows', 'symz_fold', 'eloc_fold', 'grad')
BASE_REGIONS = ('z1', 'tail_amp', 'bond_list', 'tail_eloc', 'eloc_reduce', 'grad')


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'symmetrized_bench.jsonl'))
  a = ap.parse_args(argv)
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('symmetrized_bench: no GPU')
  from cgs_vmc_amd.engine import VmcEngine
  n = SX * SY
  perms = lattice.translations(SX, SY)
  n_ops = len(perms)
  bonds = vo.torus_bonds(SX, SY)
  theta = vo.init_params(n, H, L, np.random.default_rng(1))
  cfg = vo.random_configurations(n, B, np.random.RandomState(1))
  base = VmcEngine(n, B * n_ops, L, H, seed=2024)
  base.set_params(theta)
  eng = VmcEngine.create_symmetrized(base, B, perms, None, np.full(n_ops, 1.0 / n_ops))
  eng.set_bonds(bonds, 1.0, 1.0)
  eng.set_configs(cfg)

  def step():
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.mc_steps(n, want_accepted=False)
  for _ in range(2):
    step()
  eng.synchronize()
  t0 = time.perf_counter()
  for _ in range(a.reps):
    step()
  eng.synchronize()
  step_ms = (time.perf_counter() - t0) / a.reps * 1e3
  eng.timing_enable(True); eng.timing_reset()
  base.timing_enable(True); base.timing_reset()
  for _ in range(a.reps):
    step()
  eng.synchronize()
  regions = {r: round(eng.timing_get(r)[0] / a.reps, 4) for r in REGIONS}
  base_regions = {r: round(base.timing_get(r)[0] / a.reps, 4) for r in BASE_REGIONS}
  base_ms = sum(base_regions.values())
  path = base.kernel_path()
  eng.close()
  # the base's forward alone: a plain ctx of the same shape, vmc_amplitude of its own 6,400 chains, the cache dropped first
  plain = VmcEngine(n, B * n_ops, L, H, seed=2024)
  plain.set_params(theta)
  rows = vo.random_configurations(n, B * n_ops, np.random.RandomState(2))
  amp_ms = 0.0
  for rep in range(a.reps + 2):
    plain.set_configs(rows)             # (drops the cache; synchronises)
    t0 = time.perf_counter()
    plain.amplitude()
    if rep >= 2:
      amp_ms += (time.perf_counter() - t0) * 1e3 / a.reps
  plain.close()
  forwards = n + 1
  line = dict(case='symmetrized(fully_connected 3x256) square 10x10, 100 translations', sites=n, chains=B, n_ops=n_ops,
              base_rows=B * n_ops, base_kernel_path=path, ms_per_step=round(step_ms, 3), ms_per_region=regions,
              base_ms_per_region=base_regions, base_ms_per_step=round(base_ms, 3),
              forwards_per_step=forwards, plain_amplitude_ms=round(amp_ms, 4),
              plain_amplitude_ms_x_forwards=round(amp_ms * forwards, 3),
              share_not_base_kernels=round(1.0 - min(1.0, base_ms / step_ms), 3))
  print(json.dumps(line), flush=True)
  if a.out:
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
      f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
  main()

#!/usr/bin/env python3
"""The two stochastic-reconfiguration solvers side by side on one sample store per shape: fully_connected networks on
the 10 x 10 Heisenberg torus (N = 100), 4,096 chains, 3 x 256 with 1 and 4 stored batches and 3 x 1,024 with 1 and 2.

  python tools/sr_gram_bench.py [--shapes 256:1,256:4,1024:1,1024:2] [--reps 3] [--out profiles/sr_gram_bench.jsonl]

Per shape the samples are stored once; then, alternating, engine.sr_solve (parameter space, csrc/sr.hip + srmm.hip) and
engine.sr_solve_samples (sample space, csrc/srgram.hip) run at the same diag_shift, tol = 0 and max_iter = 50, so both
run 50 iterations.  One JSON line per shape, appended to --out:
  *_solve_ms          host clock around the call (it ends in a device synchronise), median and minimum over --reps
  gram_ms             the vmc_timing region "sr_gram" (device events around k_sr_gram alone), per solve
  gram_matvec_us      the region "sr_gram_matvec" (events around one k_sr_gram_matvec), per launch
  param_matvec_ms     the region "sr_matvec" of the parameter-space solver, per iteration
  gram_tflops         executed flops of k_sr_gram (launched upper-triangle tiles x 128 x 128 x 2 x the K of every product,
                      rounded up to the 32-column chunks the kernel stages) over gram_ms, and its share of the 155 TFLOP/s
                      fp32 MFMA peak
  gram_matvec_gbs     n^2 floats over gram_matvec_us
  *_rel_residual      |r| / |rhs| of either recurrence after the 50 iterations (each in its own space)
  max_rel_diff        |x_samples - x_parameters|_inf / |x_parameters|_inf after the 50 iterations
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

PEAK_F32_MFMA = 155e12
TILE, KC = 128, 32      # SRG_TILE, SRG_KC of csrc/plan.hpp


def gram_executed_flops(n, n_sites, h, layers):
  nt = (n + TILE - 1) // TILE
  pad = lambda k: KC * ((k + KC - 1) // KC)
  k_sum = pad(n_sites) + pad(h) + (layers - 1) * 2 * pad(h) + pad(h)    # layer 0: (x, delta); hidden: (a, delta); output: a_L
  return nt * (nt + 1) // 2 * TILE * TILE * 2 * k_sum


def _wall(eng, fn, reps):
  out = []
  for _ in range(reps):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    out.append(1e3 * (time.perf_counter() - t0))
  return out


def run_shape(h, batches, args):
  from cgs_vmc_amd.engine import VmcEngine
  n_sites, layers, chains = 100, 3, args.chains
  eng = VmcEngine(n_sites, chains, layers, h, seed=2024)
  eng.set_params(vo.init_params(n_sites, h, layers, np.random.default_rng(0)))
  eng.set_configs(vo.random_configurations(n_sites, chains, np.random.RandomState(1)))
  eng.set_bonds(lattice.torus_bonds(10, 10), 1.0, 1.0)
  eng.mc_steps(4 * n_sites, want_accepted=False)
  eng.sr_reserve(batches)
  eng.reset_accumulators()
  for _ in range(batches):
    eng.accumulate(0)
    eng.mc_steps(n_sites, want_accepted=False)
  n = batches * chains
  lam, iters = args.diag_shift, args.iters
  par = lambda: eng.sr_solve(lam, 0.0, iters)
  smp = lambda: eng.sr_solve_samples(lam, 0.0, iters)
  it_par, res_par = par()                   # warm-up: code objects, the Gram matrix's allocation
  x_par = eng.sr_get_solution()
  it_smp, res_smp = smp()
  x_smp = eng.sr_get_solution()
  t_par, t_smp = [], []
  for _ in range(args.reps):          # alternating, timing regions off
    t_par += _wall(eng, par, 1)
    t_smp += _wall(eng, smp, 1)
  eng.timing_enable(True)             # the regions in a pass of their own
  eng.timing_reset()
  par(); smp()
  eng.synchronize()
  gram_ms, gram_calls = eng.timing_get('sr_gram')
  mv_ms, mv_calls = eng.timing_get('sr_gram_matvec')
  pmv_ms, pmv_calls = eng.timing_get('sr_matvec')
  eng.timing_enable(False)
  eng.close()
  flops = gram_executed_flops(n, n_sites, h, layers)
  gram_ms /= max(gram_calls, 1)
  mv_us = 1e3 * mv_ms / max(mv_calls, 1)
  return dict(network='fully_connected 3x%d' % h, sites=n_sites, chains=chains, stored_batches=batches, samples=n,
              params=int(x_par.size), diag_shift=lam, iterations=[int(it_par), int(it_smp)],
              parameters_solve_ms=dict(median=round(float(np.median(t_par)), 3), min=round(min(t_par), 3)),
              samples_solve_ms=dict(median=round(float(np.median(t_smp)), 3), min=round(min(t_smp), 3)),
              gram_ms=round(gram_ms, 4), gram_executed_gflop=round(flops / 1e9, 2),
              gram_tflops=round(flops / (gram_ms * 1e-3) / 1e12, 2) if gram_ms > 0 else None,
              gram_share_of_fp32_mfma_peak=round(flops / (gram_ms * 1e-3) / PEAK_F32_MFMA, 4) if gram_ms > 0 else None,
              gram_matvec_us=round(mv_us, 2),
              gram_matvec_gbs=round(4.0 * n * n / (mv_us * 1e-6) / 1e9, 1) if mv_us > 0 else None,
              param_matvec_ms=round(pmv_ms / max(pmv_calls, 1), 4),
              parameters_rel_residual=float(res_par), samples_rel_residual=float(res_smp),
              max_rel_diff=float(np.abs(x_smp - x_par).max() / max(np.abs(x_par).max(), 1e-30)))


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--shapes', default='256:1,256:4,1024:1,1024:2', help='units:stored batches, comma separated')
  ap.add_argument('--chains', type=int, default=4096)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--iters', type=int, default=50)
  ap.add_argument('--diag_shift', type=float, default=1e-2)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sr_gram_bench.jsonl'))
  args = ap.parse_args(argv)
  lines = []
  for item in args.shapes.split(','):
    h, batches = (int(v) for v in item.split(':'))
    line = run_shape(h, batches, args)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
      os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
      with open(args.out, 'a') as f:
        f.write(text + '\n')
    lines.append(line)
  return lines


if __name__ == '__main__':
  main()

"""CPU: the sample-space stochastic reconfiguration without a GPU -- the per-layer Gram formula and the n x n solve of
tests/sr_gram_cases.py against the oracle's explicit per-sample gradients and dense solve, the planner of the Gram launch
(plan.hpp: plan_sr_gram*) under AddressSanitizer + UndefinedBehaviourSanitizer in a program of its own
(csrc/hostcheck_srgram.cpp), and the solver switch of parallel.sr_solve."""
import os
import re
import subprocess

import numpy as np
import pytest

from cgs_vmc_amd import parallel
from oracle import vmc_oracle as vo
from tests import sr_gram_cases as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, H, L, n): the shapes the identity was checked at
IDENTITY_SHAPES = [(16, 32, 2, 192), (12, 40, 1, 96), (10, 30, 2, 74), (8, 16, 2, 24)]


@pytest.mark.parametrize('ansatz', ['fully_connected', 'rbm'])
@pytest.mark.parametrize('n,h,L,rows', [(8, 16, 2, 24), (10, 30, 2, 74)])
def test_gram_formula_matches_explicit_gradients(ansatz, n, h, L, rows):
  theta, cfgs = sg.make_case(ansatz, n, h, L, rows, seed=1)
  o = sg.per_sample_grads(theta, cfgs, h, L, ansatz)
  ref = o @ o.T
  got = sg.gram_ref(theta, cfgs, h, L, ansatz)
  assert got.shape == (rows, rows)
  assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize('n,h,L,rows', IDENTITY_SHAPES)
def test_sample_space_solve_matches_dense_solve(n, h, L, rows):
  theta, cfgs = sg.make_case('fully_connected', n, h, L, rows, seed=2)
  o = sg.per_sample_grads(theta, cfgs, h, L)
  amp = lambda c: vo.fc_psi(theta, c, h, L, dtype=np.float64)
  e = np.asarray(vo.local_value(amp, cfgs, vo.chain_bonds(n), -1.0, 1.0, dtype=np.float64), np.float64)
  assert e.std() > 0
  lam = 1e-2
  ref = vo.sr_solve(o, e, lam)
  got = sg.solve_samples_ref(o, e, lam)
  assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max()
  # the fp64 CG of the helper reaches the same solution through T alone
  t_w, it = sg.cg_samples_ref(sg.gram_ref(theta, cfgs, h, L), e, lam, 1e-10, 2000)
  assert it > 0 and np.abs(o.T @ t_w - ref).max() <= 1e-7 * np.abs(ref).max()


def test_gram_planner_under_asan_and_ubsan():
  p = subprocess.run(['make', '-C', os.path.join(ROOT, 'cgs_vmc_amd', 'csrc'), 'hostcheck_srgram'],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
  out = p.stdout.decode()
  assert p.returncode == 0, out[-4000:]
  assert '-fsanitize=address,undefined' in out
  assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
  m = re.search(r'hostcheck_srgram ok: (\d+) cases, (\d+) assertions', out)
  assert m, out[-2000:]
  # n = 1 .. 300 and the five large sizes; every case asserts at least its return code and one tile
  assert int(m.group(1)) == 305 and int(m.group(2)) >= 2 * 305


class _Untouchable:
  """An engine no refusal may reach."""

  def __getattr__(self, name):
    raise AssertionError('the engine was touched: ' + name)


def test_sr_solve_rejects_unknown_solver():
  with pytest.raises(ValueError, match='bogus'):
    parallel.sr_solve(_Untouchable(), 1e-2, 1e-3, 10, solver='bogus')


def test_sr_solve_samples_needs_one_rank(monkeypatch):
  monkeypatch.setattr(parallel, 'world_size', lambda: 2)
  with pytest.raises(NotImplementedError, match='all-gather'):
    parallel.sr_solve(_Untouchable(), 1e-2, 1e-3, 10, solver='samples')

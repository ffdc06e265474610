"""CPU: the sample-space stochastic reconfiguration without a GPU -- the per-layer Gram formula and the n x n solve of
tests/sr_gram_cases.py against the oracle's explicit per-sample gradients and dense solve, the planner of the Gram launch
(plan.hpp: plan_sr_gram*) under AddressSanitizer + UndefinedBehaviourSanitizer in a program of its own
(csrc/hostcheck_srgram.cpp), the solver switch of parallel.sr_solve, and the inputs of tests/test_gpu_sr_gram_shapes.py
(tests/sr_gram_shape_cases.py): what the GPU tests take for granted about them is measured here on the fp64 references."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from cgs_vmc_amd import parallel
from oracle import vmc_oracle as vo
from tests import sr_gram_cases as sg
from tests import sr_gram_shape_cases as ssc

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
  # n = 1 .. 300, 1,024 and the four sizes of tests/sr_gram_shape_cases.py above 300, and the five large sizes; every
  # case asserts at least its return code and one tile
  assert {n for n in ssc.ROWS.values() if n > 300} == {516, 1025, 1040, 1100}
  assert int(m.group(1)) == 310 and int(m.group(2)) >= 2 * 310


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


# ---------------------------------------------------------------------------- the helpers of the shape tests
@pytest.mark.parametrize('ansatz,nonlin', [('fully_connected', 'relu'), ('fully_connected', 'cos'), ('rbm', 'relu'),
                                           ('rbm', 'tanh')])
def test_per_sample_grads_from_terms_is_the_oracles(ansatz, nonlin):
  theta, cfgs = sg.make_case(ansatz, 10, 30, 2, 37, seed=4)
  ref = sg.per_sample_grads(theta, cfgs, 30, 2, ansatz, nonlin)
  got = sg.per_sample_grads_from_terms(theta, cfgs, 30, 2, ansatz, nonlin)
  assert got.shape == ref.shape and got.dtype == np.float64
  assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize('ansatz', ['fully_connected', 'rbm'])
@pytest.mark.parametrize('nonlin', ['relu', 'tanh', 'sigmoid', 'cos'])
def test_gram_magnitude_and_fp32_formula(ansatz, nonlin):
  """M is the sum of the absolute products behind O O^T: it bounds |T|, equals T where no product is negative (every
  parameter's derivative squared: the diagonal), and the fp32 evaluation is fp32 and within a few eps of it."""
  theta, cfgs = sg.make_case(ansatz, 10, 30, 2, 74, seed=5)
  o = sg.per_sample_grads(theta, cfgs, 30, 2, ansatz, nonlin)
  m = sg.gram_magnitude(theta, cfgs, 30, 2, ansatz, nonlin)
  t = sg.gram_ref(theta, cfgs, 30, 2, ansatz, nonlin)
  assert m.dtype == np.float64 and np.all(m >= np.abs(t))
  assert np.abs(np.diag(m) - np.diag(t)).max() <= 1e-12 * np.diag(t).max()
  # ... and it is no looser than it says: the factored |a||a|^T o |d||d|^T is the plain sum over the parameters
  assert np.abs(m - np.abs(o) @ np.abs(o).T).max() <= 1e-12 * m.max()
  t32 = sg.gram_fp32(theta, cfgs, 30, 2, ansatz, nonlin)
  assert t32.dtype == np.float32 and t32.shape == t.shape
  assert (np.abs(t32 - t) / m).max() <= 1e-6


def test_cg_history_is_the_truncated_recurrence():
  theta, cfgs = sg.make_case('fully_connected', 10, 30, 2, 74, seed=6)
  t = sg.gram_ref(theta, cfgs, 30, 2)
  e = np.random.default_rng(1).standard_normal(74)
  plain = sg.cg_samples_ref(t, e, 1e-2, 1e-6, 2000)
  assert len(plain) == 2                               # the callers before the history keep their pair
  w, it, hist = sg.cg_samples_ref(t, e, 1e-2, 1e-6, 2000, history=True)
  assert it == plain[1] > 13 and np.array_equal(w, plain[0])
  assert len(hist) == it + 1 and hist[0][1] == 1.0 and not hist[0][0].any()
  assert np.array_equal(hist[it][0], w) and hist[it][1] <= 1e-6 < hist[it - 1][1]
  for k in (0, 1, 3, 8, 13):
    wk, itk = sg.cg_samples_ref(t, e, 1e-2, 1e-6, k)
    assert itk == k and np.array_equal(wk, hist[k][0])
    assert abs(hist[k][0].mean()) <= 1e-15 * max(1.0, np.abs(hist[k][0]).max())


def test_draw_rows_keeps_relu_rows_off_the_kink():
  theta = sg.make_theta('fully_connected', 16, 33, 3)
  cfgs, rejected = sg.draw_rows('fully_connected', theta, 16, 33, 3, 400, 3, 'relu')
  plain = vo.random_configurations(16, 400, np.random.RandomState(3))
  assert cfgs.shape == (400, 16) and cfgs.dtype == np.float32 and np.all(cfgs.sum(1) == 0)
  assert sg.min_preactivation(theta, cfgs, 33, 3).min() >= sg.KINK
  near = sg.min_preactivation(theta, plain, 33, 3) < sg.KINK
  assert rejected >= near.sum() and np.array_equal(cfgs[~near], plain[~near])      # only the rows at the kink were redrawn
  again, rejected2 = sg.draw_rows('fully_connected', theta, 16, 33, 3, 400, 3, 'relu')
  assert rejected2 == rejected and np.array_equal(again, cfgs)
  smooth, none = sg.draw_rows('fully_connected', theta, 16, 33, 3, 400, 3, 'tanh')
  assert none == 0 and np.array_equal(smooth, plain)                               # a smooth activation takes every row


# ---------------------------------------------------------------------------- the inputs of the shape tests
def test_shape_cases_reach_what_their_rows_promise():
  c, rows = ssc.CASES, ssc.ROWS
  assert all(n <= 1100 for n in rows.values()) and ssc.N == 16
  assert rows['full128'] == ssc.TILE
  assert rows['one_over'] == ssc.TILE + 1
  for cid in ('big_deep', 'tanh1100'):
    n, s = rows[cid], c[cid]
    assert n == 1100 > ssc.LOOP and -(-n // ssc.TILE) == 9 and n % ssc.TILE == 76
    assert s.reserved * s.b == 1375 != n                       # row stride != rows
    assert s.h == ssc.CHUNK + 1 and s.L + 1 == 4               # one column past a chunk; four layer terms
    assert n % 4 == 0 and n // 4 > 64                          # the float4 matvec, a second trip per lane
  assert c['tanh1100'] == c['big_deep']._replace(act='tanh')
  n = rows['odd1025']
  assert n == ssc.LOOP + 1 and n % 4 != 0 and -(-n // 64) == 17
  n = rows['rbm1040']
  assert c['rbm1040'].ansatz == 'rbm' and -(-n // ssc.TILE) == 9 and n > ssc.LOOP and n % 4 == 0
  for cid in ('sig516', 'cos516'):
    assert rows[cid] == 516 and -(-516 // ssc.TILE) == 5 and 516 % ssc.TILE == 4 and c[cid].b % 2 == 1
  assert {s.act for s in c.values()} == {'relu', 'tanh', 'sigmoid', 'cos'}
  assert all(s.stored <= s.reserved for s in c.values())
  assert max(ssc.TRUNCATIONS) == 13 and {0, 8, 9} <= set(ssc.TRUNCATIONS)      # none, a group boundary, one past it
  assert all(ssc.gram_c(cid) <= ssc.GRAM_GLOBAL for cid in ssc.IDS)
  src = open(os.path.join(ROOT, 'cgs_vmc_amd', 'csrc', 'plan.hpp')).read()
  assert re.search(r'#define\s+SRG_TILE\s+{}\b'.format(ssc.TILE), src)
  assert re.search(r'#define\s+SRG_KC\s+{}\b'.format(ssc.CHUNK), src)
  assert 'i += {})'.format(ssc.LOOP) in open(os.path.join(ROOT, 'cgs_vmc_amd', 'csrc', 'srgram.hip')).read()


@functools.lru_cache(maxsize=None)
def _measured(cid):
  """What the CPU can say about a case: the oracle's fp64 local energies stand in for the engine's."""
  s = ssc.CASES[cid]
  theta, cfgs, rejected = ssc.inputs(cid)
  args = (theta, cfgs, s.h, s.L, s.ansatz, s.act)
  t, m = sg.gram_ref(*args), sg.gram_magnitude(*args)
  psi = vo.rbm_psi if s.ansatz == 'rbm' else vo.fc_psi
  amp = lambda c: psi(theta, c, s.h, s.L, nonlinearity=s.act, dtype=np.float64)
  e = np.asarray(vo.local_value(amp, cfgs, vo.chain_bonds(ssc.N), -1.0, 1.0, dtype=np.float64), np.float64)
  return dict(t=t, m=m, e=e, rejected=rejected, ratio=float((np.abs(sg.gram_fp32(*args) - t) / m).max()),
              it64=sg.cg_samples_ref(t, e, ssc.LAM, 1e-6, 2000)[1])


@pytest.mark.parametrize('cid', ssc.IDS)
def test_shape_case_inputs(cid):
  s, n = ssc.CASES[cid], ssc.ROWS[cid]
  theta, cfgs, rejected = ssc.inputs(cid)
  got = _measured(cid)
  distinct = np.unique(cfgs, axis=0).shape[0]
  print(cid, 'n', n, 'rejected', rejected, 'distinct', distinct, 'fp32 ratio', got['ratio'], 'it64', got['it64'])
  assert cfgs.shape == (n, ssc.N) and np.all(cfgs.sum(1) == 0)
  assert sum(b.shape[0] for b in ssc.batches(cid)) == n and all(b.shape[0] == s.b for b in ssc.batches(cid))
  assert rejected <= 0.05 * (n + rejected)
  assert (rejected == 0) or s.act == 'relu'
  if s.act == 'relu':
    assert sg.min_preactivation(theta, cfgs, s.h, s.L, s.ansatz).min() >= sg.KINK
  assert distinct >= 0.9 * n
  assert np.all(got['m'] >= np.abs(got['t']))
  assert got['e'].std() > 0
  # plain fp32 arithmetic against fp64, relative to the magnitude sum: the recorded figure, which the GPU bound scales
  assert ssc.FP32_RATIO[cid] / ssc.FP32_ROOM <= got['ratio'] <= ssc.FP32_RATIO[cid] * ssc.FP32_ROOM
  if cid in ssc.STOP_CASES:
    assert got['it64'] >= 20 and got['it64'] > max(ssc.TRUNCATIONS) + 8      # every truncation lies strictly inside

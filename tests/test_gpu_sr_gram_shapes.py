"""GPU: the sample-space stochastic reconfiguration (cgs_vmc_amd/csrc/srgram.hip) past the 300 samples and the three tiles
a side of tests/test_gpu_sr_gram.py -- full and one-sample tile rows, nine tiles a side, a second trip of every
single-workgroup loop and of the matvec's lanes, four layer terms, the deltas of every hidden activation, the stop of
the conjugate gradients to the iteration, solves cut short by max_iter, and a store that grows and shrinks on one ctx.
Inputs: tests/sr_gram_shape_cases.py (checked on the CPU by tests/test_sr_gram.py); references: tests/sr_gram_cases.py
in fp64.

Tolerances:
  Gram matrix, per element   |T - T_ref| <= c M, M the sum of the absolute products behind the entry
                             (sr_gram_cases.gram_magnitude), c = 16 x the worst |d| / M of a plain numpy fp32 evaluation
                             of the same formula (sr_gram_shape_cases.FP32_RATIO, re-measured by tests/test_sr_gram.py)
  Gram matrix, global        |d| <= 2e-4 max|T_ref| (tests/test_gpu_sr_gram.py's, kept beside the other)
  CG solution, iterates      |d| <= 2e-3 ||x_ref||_inf, residuals 2e-3 relative; both solvers 4e-3 (the same file's)
"""
import numpy as np
import pytest

from oracle import vmc_oracle as vo
from tests import sr_gram_cases as sg
from tests import sr_gram_shape_cases as ssc

pytestmark = pytest.mark.gpu

LAM = ssc.LAM
TOL = 1e-6


class Case:
  pass


_CASES = {}


def _engine(cid):
  """A fresh engine of a case: parameters set, store reserved and empty."""
  from cgs_vmc_amd.engine import VmcEngine
  s = ssc.CASES[cid]
  eng = VmcEngine(ssc.N, s.b, s.L, s.h, seed=2024, ansatz=s.ansatz, nonlinearity=s.act)
  eng.set_params(ssc.inputs(cid)[0])
  eng.set_bonds(vo.chain_bonds(ssc.N), -1.0, 1.0)
  eng.sr_reserve(s.reserved)
  eng.reset_accumulators()
  return eng


def _record(eng, cfg):
  """One batch into the store; the local energies the engine recorded with it."""
  eng.set_configs(cfg)
  eng.accumulate(0)
  return eng.local_energy()[0]


def _case(cid):
  """The engine with its store filled, and the fp64 references, once per case (the references are never written)."""
  if cid in _CASES:
    return _CASES[cid]
  s = ssc.CASES[cid]
  c = Case()
  c.cid, c.s = cid, s
  c.theta, c.cfgs, _ = ssc.inputs(cid)
  c.eng = _engine(cid)
  c.e = np.concatenate([_record(c.eng, b) for b in ssc.batches(cid)], 0).astype(np.float64)
  assert c.eng.sr_num_stored() == s.stored
  args = (c.theta, c.cfgs, s.h, s.L, s.ansatz, s.act)
  c.t_ref, c.m = sg.gram_ref(*args), sg.gram_magnitude(*args)
  c.o = sg.per_sample_grads_from_terms(*args)
  c.x_ref = sg.solve_samples_ref(c.o, c.e, LAM)
  _, c.it64, c.hist = sg.cg_samples_ref(c.t_ref, c.e, LAM, TOL, 2000, history=True)
  for a in (c.e, c.t_ref, c.m, c.o, c.x_ref):
    a.setflags(write=False)
  c.full = None
  _CASES[cid] = c
  return c


def _solve(c, max_iter):
  iters, res = c.eng.sr_solve_samples(LAM, TOL, max_iter)
  return iters, res, c.eng.sr_get_solution()


def _full(c):
  """(iterations, residual, x) of the solve that runs to its stop, once per case."""
  if c.full is None:
    c.full = _solve(c, 2000)
    c.full[2].setflags(write=False)
  return c.full


@pytest.mark.parametrize('cid', ssc.IDS)
def test_gram_per_element(cid):
  """Every entry of T within c M of fp64, c = 16 x the CPU's fp32 figure; T symmetric and repeatable bit for bit.

  case       CPU fp32 worst |d| / M    c          device worst |d| / (c M), measured on an MI355X
  full128    2.63e-7                   4.21e-6    0.045
  one_over   2.63e-7                   4.21e-6    0.045   (its first 128 rows are full128's)
  big_deep   3.59e-7                   5.74e-6    0.056
  odd1025    2.59e-7                   4.14e-6    0.064
  rbm1040    3.43e-7                   5.49e-6    0.066
  tanh1100   2.78e-7                   4.45e-6    0.057
  sig516     2.76e-7                   4.42e-6    0.064
  cos516     3.46e-7                   5.54e-6    0.058
  The device's worst |d| / M is 1.9e-7 .. 3.6e-7: what plain fp32 arithmetic leaves on the CPU, for every activation; the
  factor 16 is not used up anywhere, so no activation needed a tolerance of its own.
  """
  c = _case(cid)
  n = ssc.ROWS[cid]
  bound = ssc.gram_c(cid)
  assert bound <= ssc.GRAM_GLOBAL
  t = c.eng.sr_debug_gram()
  assert t.shape == (n, n) and t.dtype == np.float32
  assert np.all(np.isfinite(t))
  d = np.abs(t - c.t_ref)
  ratio = d / (bound * c.m)
  r, q = np.unravel_index(np.argmax(ratio), ratio.shape)
  print('gram', cid, 'n', n, 'fp32 ratio', ssc.FP32_RATIO[cid], 'c', bound, 'worst |d|/(c M)', ratio[r, q], 'row', r, 'col', q,
        'tile', (r // ssc.TILE, q // ssc.TILE), '|d|/M', d[r, q] / c.m[r, q], 'global', d.max() / np.abs(c.t_ref).max())
  assert np.array_equal(t, t.T)
  assert np.array_equal(t, c.eng.sr_debug_gram())
  assert d.max() <= ssc.GRAM_GLOBAL * np.abs(c.t_ref).max()
  assert ratio[r, q] <= 1.0, (r, q, t[r, q], c.t_ref[r, q], c.m[r, q])


@pytest.mark.parametrize('cid', ssc.IDS)
def test_solution_matches_direct_solve(cid):
  """cond(C T C + n lambda I) is 3 (sigmoid) .. 650 (rbm1040: above the 90 .. 200 of tests/test_gpu_sr_gram.py)."""
  c = _case(cid)
  iters, res, x = _full(c)
  err, scale = np.abs(x - c.x_ref).max(), np.abs(c.x_ref).max()
  print('solve', cid, 'iters', iters, 'it64', c.it64, 'res', res, 'err/scale', err / scale)
  assert res <= 1e-4, (iters, res)
  assert np.all(np.isfinite(x))
  assert err <= 2e-3 * scale, (iters, res)
  assert abs(iters - c.it64) <= 2             # (not the 2 it64 + 10 of tests/test_gpu_sr_gram.py: the vectors are fp64)
  ref = vo.sr_solve(c.o, c.e, LAM)         # dense fp64 solve of the explicit (S + lam I)
  assert np.abs(x - ref).max() <= 2e-3 * np.abs(ref).max()
  iters2, res2, x2 = _solve(c, 2000)
  assert iters2 == iters and res2 == res and np.array_equal(x2, x)


@pytest.mark.parametrize('cid', ssc.AGREE_CASES)
def test_agrees_with_parameter_space_solver(cid):
  c = _case(cid)
  x = _full(c)[2]
  c.eng.sr_solve(LAM, TOL, 2000)
  x_par = c.eng.sr_get_solution()
  err, scale = np.abs(x - x_par).max(), np.abs(x_par).max()
  print('agree', cid, 'err/scale', err / scale)
  assert err <= 4e-3 * scale


@pytest.mark.parametrize('cid', ssc.EXACT_STOP_CASES)
def test_the_stop_is_exact(cid):
  """The solve stops at the first iteration that meets |r| <= tol |eps| and at no later one: the iterations the host has
  enqueued behind it, to the end of its group of 8, change nothing, whatever max_iter leaves of the group.  Measured
  stops: full128 39, one_over 40, big_deep 29 -- one_over's is the end of a group, where the host's read alone ends the
  solve; the other two have one and three iterations enqueued behind theirs."""
  c = _case(cid)
  it, res, x = _full(c)
  print('stop', cid, 'it', it, 'it64', c.it64, 'res', res)
  assert res <= TOL
  assert it % 8 != 0 or cid == 'one_over'    # iterations behind the stop in the 2000-iteration run itself
  assert abs(it - c.it64) <= 2               # (the fp32 and the fp64 residual may straddle the threshold)
  for more in (0, 1, 8):
    it2, res2, x2 = _solve(c, it + more)
    assert (it2, res2) == (it, res), more
    assert np.array_equal(x2, x), more
  it3, res3, x3 = _solve(c, it - 1)
  print('stop', cid, 'one short: res', res3)
  assert it3 == it - 1 and res3 > TOL        # the criterion was not met an iteration earlier
  assert not np.array_equal(x3, x)


@pytest.mark.parametrize('k', ssc.TRUNCATIONS)
@pytest.mark.parametrize('cid', ssc.STOP_CASES)
def test_truncated_solve_follows_the_fp64_recurrence(cid, k):
  c = _case(cid)
  assert k < c.it64 - 2
  iters, res, x = _solve(c, k)
  assert iters == k
  if k == 0:
    assert res == 1.0 and not x.any()
    try:
      assert np.isfinite(c.eng.sr_apply(0.05))
      assert np.array_equal(c.eng.get_params(), c.theta)
    finally:
      c.eng.set_params(c.theta)
    return
  w_k, res_k = c.hist[k]
  x_k = c.o.T @ w_k
  err, scale = np.abs(x - x_k).max(), np.abs(x_k).max()
  print('truncated', cid, 'k', k, 'err/scale', err / scale, 'res', res, 'res64', res_k, 'rel', abs(res - res_k) / res_k)
  assert np.all(np.isfinite(x))
  assert err <= 2e-3 * scale
  assert abs(res - res_k) <= 2e-3 * res_k


def test_store_grows_and_shrinks_on_one_ctx():
  """sr_gram and the CG vectors are reserved by the first solve that needs them: one batch (n = 275), four (n = 1100, the
  buffers grown: the bits of the engine that only ever saw four), one again (the larger buffers still there: the bits of
  the first solve, so nothing reads past n)."""
  cid = ssc.GROW_CASE
  c = _case(cid)
  it_ref, res_ref, x_ref = _full(c)
  t_ref = c.eng.sr_debug_gram()
  b = ssc.batches(cid)
  eng = _engine(cid)
  e0 = _record(eng, b[0])
  first = eng.sr_solve_samples(LAM, TOL, 2000)
  x_first, t_first = eng.sr_get_solution(), eng.sr_debug_gram()
  assert t_first.shape == (c.s.b, c.s.b) and first[1] <= 1e-4
  assert np.array_equal(t_first, t_ref[:c.s.b, :c.s.b])
  # (the small solve is a solve: against fp64 as everywhere)
  small = sg.solve_samples_ref(c.o[:c.s.b], e0.astype(np.float64), LAM)
  assert np.abs(x_first - small).max() <= 2e-3 * np.abs(small).max()
  for k in range(1, c.s.stored):
    _record(eng, b[k])
  assert eng.sr_solve_samples(LAM, TOL, 2000) == (it_ref, res_ref)
  assert np.array_equal(eng.sr_get_solution(), x_ref)
  assert np.array_equal(eng.sr_debug_gram(), t_ref)
  eng.reset_accumulators()
  assert np.array_equal(_record(eng, b[0]), e0)
  assert eng.sr_solve_samples(LAM, TOL, 2000) == first
  assert np.array_equal(eng.sr_get_solution(), x_first)
  assert np.array_equal(eng.sr_debug_gram(), t_first)
  eng.close()

"""CPU: the overlap estimator and the penalised gradient (tests/overlap_cases.py) against dense linear algebra on the 8-site
chain, OverlapEvaluator on a scripted engine, the optimizer registry and argument checks, the lower-state checkpoint check
and the drivers' file round trips.  The GPU side is tests/test_gpu_state_overlap.py."""
import os
import types

import numpy as np
import pytest

from cgs_vmc_amd import evaluation, parallel, session as session_lib, training, utils, wavefunctions
from tests import moments_oracle as mo
from tests import overlap_cases as oc

N = 8
BONDS = [(i, (i + 1) % N) for i in range(N)]


@pytest.fixture(autouse=True)
def _fresh_graph():
  session_lib.reset_default_graph()
  wavefunctions.reset_name_scope()
  yield


# ---- estimator math on the enumerated Sz = 0 sector

def _table_states(seed=11):
  rng = np.random.default_rng(seed)
  basis, h = mo.dense_h(N, BONDS, 1.0, 1.0)
  assert len(basis) == 70
  return h, rng.uniform(0.2, 1.5, 70), rng.uniform(0.2, 1.5, 70)


def _ratios_of(psi, phi):
  # a table ansatz: the "logit" is ln psi, no shift, no sign buffer
  return oc.Ratios(np.log(phi) - np.log(psi), np.ones(len(psi), np.int64), np.ones(len(psi), bool))


def _objective(h, psi, phi, lam):
  e = psi @ h @ psi / (psi @ psi)
  f = (phi @ psi) ** 2 / ((psi @ psi) * (phi @ phi))
  return e + lam * f


def test_sums_fidelity_is_the_dense_fidelity():
  h, psi, phi = _table_states()
  p = psi ** 2 / (psi ** 2).sum()
  dense = (phi @ psi) ** 2 / ((psi @ psi) * (phi @ phi))
  assert abs(oc.fidelity(_ratios_of(psi, phi), weight=p) - dense) <= 1e-12
  # the scale of phi is arbitrary: 1e+-120 moves log_scale and nothing else
  for scale in (1e120, 1e-120):
    v = oc.sums(_ratios_of(psi, scale * phi), weight=p)
    assert abs(v['s1'] ** 2 / (v['alive'] * v['s2']) - dense) <= 1e-12
    assert np.isfinite(v['s1']) and v['s2'] > 0


def test_penalized_gradient_is_the_finite_difference_of_the_objective():
  h, psi, phi = _table_states()
  lam = 1.7
  p = psi ** 2 / (psi ** 2).sum()
  eloc = (h @ psi) / psi
  w = oc.weights(eloc, _ratios_of(psi, phi), lam, weight=p, dtype=np.float64)
  # O_k(x) = delta(k, x) / psi_k: 2 Cov(w, O)_k = 2 p_k (w_k - <w>) / psi_k
  grad = 2.0 * p * (w - (p * w).sum()) / psi
  step = 1e-6
  fd = np.empty(70)
  for k in range(70):
    up, dn = psi.copy(), psi.copy()
    up[k] += step; dn[k] -= step
    fd[k] = (_objective(h, up, phi, lam) - _objective(h, dn, phi, lam)) / (2 * step)
  assert np.abs(grad - fd).max() <= 1e-6 * np.abs(fd).max()
  # the accumulator form: g1 = sum O, g2 = sum w O over the same weights, no factor 2
  g1, g2 = p / psi, p * w / psi
  np.testing.assert_allclose(2.0 * oc.penalized_gradient(g1, g2, (p * w).sum(), (1.0, 1.0)), grad, rtol=1e-12, atol=1e-15)


def test_dead_chains_and_vanishing_phi_in_the_restatement():
  # chain 1 is dead (psi = 0), chain 2 has phi = 0: ratio 0, alive
  r = oc.ratios(np.float32([0.5, -np.inf, 0.25, 1.0]), np.float32([1, 0, -1, 1]), 0.0,
                np.float32([1.0, 0.3, -np.inf, 0.5]), np.float32([1, 1, 0, -1]), 0.0)
  assert list(r.s) == [1, 0, 0, -1] and list(r.alive) == [True, False, True, True]
  v = oc.sums(r)
  assert v['alive'] == 3 and v['log_scale'] == 0.5
  np.testing.assert_allclose(v['ratio'], [1.0, 0.0, 0.0, -np.exp(-1.0)], rtol=1e-15)
  w = oc.weights(np.float32([1, 2, 3, 4]), r, 2.0)
  assert w.dtype == np.float32 and w[1] == 2.0 and w[2] == 3.0
  none = oc.sums(oc.ratios(np.float32([0.0]), np.float32([1]), 0.0, np.float32([0.0]), np.float32([0]), 0.0))
  assert none['s2'] == 0 and none['log_scale'] == 0.0
  assert oc.fidelity(oc.ratios(np.float32([0.0]), np.float32([1]), 0.0, np.float32([0.0]), np.float32([0]), 0.0)) == 0.0


# ---- the evaluator on a scripted engine

class _ScriptedEngine:
  """Engine double: overlap returns the next scripted sums; run_many counts the sampler's calls."""

  def __init__(self, script):
    self.script, self.at, self.steps = list(script), 0, []

  def overlap(self, per_chain=False):
    assert not per_chain
    s = self.script[self.at]
    self.at += 1
    return {'s1': s[0], 's2': s[1], 'alive': int(s[2]), 'log_scale': s[3]}

  def run_many(self, n):
    self.steps.append(n)


def _ops(engine):
  mc = session_lib.Op(lambda: None, 'mc_step')
  mc.last_accepted = 3
  mc.run_many = engine.run_many
  return evaluation.EvalOps(value=evaluation.OverlapTensor(engine), mc_step=mc, acceptance_rate=None,
                            placeholder_input=None, wavefunction_value=None)


def _hparams(n_samples, batch=64):
  return types.SimpleNamespace(num_sites=8, batch_size=batch, num_equilibration_sweeps=5, num_monte_carlo_sweeps=2,
                               num_evaluation_samples=n_samples)


def _script(scales, seed=4, batch=64):
  """Per sample (s1, s2, alive, log_scale) of `batch` ratios exp(d), d ~ N(scale, 0.3), a tenth of them negative; and
  the ln|r| and signs behind them."""
  rng = np.random.default_rng(seed)
  script, logs, signs = [], [], []
  for scale in scales:
    d = scale + 0.3 * rng.standard_normal(batch)
    s = np.where(rng.uniform(size=batch) < 0.1, -1, 1)
    m = d.max()
    script.append(((s * np.exp(d - m)).sum(), np.exp(2 * (d - m)).sum(), batch, m))
    logs.append(d); signs.append(s)
  return script, np.array(logs), np.array(signs)


def _log_domain_fidelity(logs, signs):
  """(sum r)^2 / (n sum r^2) with every sum taken through fp64 logarithms (log-sum-exp, the two signs apart)."""
  d, s = logs.ravel(), signs.ravel()
  lse = lambda x: x.max() + np.log(np.exp(x - x.max()).sum()) if len(x) else -np.inf
  lp, ln_, l2 = lse(d[s > 0]), lse(d[s < 0]), lse(2 * d)
  hi = max(lp, ln_)
  s1 = np.exp(lp - hi) - np.exp(ln_ - hi)                # in units of exp(hi)
  return s1 * s1 * np.exp(2 * hi - l2) / len(d)


@pytest.mark.parametrize('scales', [(0.0, 0.4, -0.7, 0.1), (3.0, 5.5, -2.0), (300.0, 0.0, -300.0, 299.5)])
def test_evaluator_combines_samples_at_different_scales(scales):
  script, logs, signs = _script(scales)
  eng = _ScriptedEngine(script)
  ev = evaluation.OverlapEvaluator()
  out = ev.run_evaluation(_ops(eng), session_lib.Session(), _hparams(len(scales)), epoch_num=0)
  assert eng.at == len(scales) and eng.steps == [5 * 8] + [2 * 8] * len(scales) and ev.acceptance_count == 3 * len(scales)
  assert set(out) == {'fidelity', 'fidelity_err', 'overlap_sign', 'alive_fraction', 'samples'}
  np.testing.assert_array_equal(out['samples'], np.array(script, np.float64))
  np.testing.assert_allclose(out['fidelity'], _log_domain_fidelity(logs, signs), rtol=1e-12)
  assert np.isfinite(out['fidelity_err']) and out['overlap_sign'] == 1.0 and out['alive_fraction'] == 1.0


def test_evaluator_jackknife_against_a_delete_one_loop():
  scales = (0.0, 0.4, -0.7, 0.1, 0.3)
  script, logs, signs = _script(scales, seed=9)
  out = evaluation.OverlapEvaluator().run_evaluation(_ops(_ScriptedEngine(script)), session_lib.Session(),
                                                     _hparams(len(scales)), epoch_num=0)
  n = len(scales)
  left = np.array([_log_domain_fidelity(np.delete(logs, t, 0), np.delete(signs, t, 0)) for t in range(n)])
  err = np.sqrt((n - 1.0) / n * ((left - left.mean()) ** 2).sum())
  np.testing.assert_allclose(out['fidelity_err'], err, rtol=1e-9)
  single = evaluation.OverlapEvaluator().run_evaluation(_ops(_ScriptedEngine(script[:1])), session_lib.Session(),
                                                        _hparams(1), epoch_num=0)
  assert single['fidelity_err'] == 0.0


def test_vanishing_phi_gives_fidelity_zero_not_nan():
  assert evaluation.fidelity_from_sums(0.0, 0.0, 64) == 0.0
  assert evaluation.fidelity_from_sums(0.0, 0.0, 0) == 0.0
  script = [(0.0, 0.0, 60, 0.0), (0.0, 0.0, 64, 0.0)]
  out = evaluation.OverlapEvaluator().run_evaluation(_ops(_ScriptedEngine(script)), session_lib.Session(), _hparams(2),
                                                     epoch_num=0)
  assert out['fidelity'] == 0.0 and out['fidelity_err'] == 0.0 and out['overlap_sign'] == 0.0
  assert out['alive_fraction'] == 124 / 128
  # one sample without a ratio among others that hold one: its scale is not read
  mixed = evaluation.overlap_common_scale([(0.0, 0.0, 64, 0.0), (3.0, 5.0, 64, 700.0)])
  np.testing.assert_array_equal(mixed, [[0.0, 0.0, 64.0], [3.0, 5.0, 64.0]])


# ---- registries and the optimizer's argument checks

def test_registries():
  assert set(training.EXCITED_STATE_OPTIMIZERS) == {'PenalizedEnergyGradient'}
  assert training.EXCITED_STATE_OPTIMIZERS['PenalizedEnergyGradient'] is training.PenalizedEnergyGradientOptimizer
  assert issubclass(training.PenalizedEnergyGradientOptimizer, training.EnergyGradientOptimizer)
  assert set(training.GROUND_STATE_OPTIMIZERS) == {'EnergyGradient', 'LogOverlapITSWO', 'ITSWO', 'StochasticReconfiguration'}


class _NeverBound:
  """A wavefunction stand-in that fails the test when an engine is asked for."""

  def _bind(self, configs):
    raise AssertionError('an engine was asked for')


def test_optimizer_argument_checks(monkeypatch):
  hp = utils.create_hparams(num_sites=8, batch_size=16)
  opt = training.PenalizedEnergyGradientOptimizer()
  with pytest.raises(ValueError, match='overlap_penalty'):
    opt.build_opt_ops(_NeverBound(), None, hp, {})
  for bad in (0.0, -1.5, float('nan'), float('inf')):
    hp.overlap_penalty = bad
    with pytest.raises(ValueError, match='overlap_penalty'):
      opt.build_opt_ops(_NeverBound(), None, hp, {})
  hp.overlap_penalty = 2.0
  monkeypatch.setattr(parallel, 'is_distributed', lambda: True)
  with pytest.raises(NotImplementedError, match='one rank'):
    opt.build_opt_ops(_NeverBound(), None, hp, {})
  with pytest.raises(NotImplementedError, match='one rank'):
    evaluation.OverlapEvaluator().build_eval_ops(_NeverBound(), _NeverBound(), hp, {})


# ---- the lower state's checkpoint

def _checkpoint(directory, fc_layer_size):
  wavefunctions.reset_name_scope()               # every run directory holds the names of a first wavefunction
  hp = utils.create_hparams(num_sites=8, wavefunction_type='fully_connected', fc_layer_size=fc_layer_size, num_fc_layers=2)
  wf = wavefunctions.build_wavefunction(hp)
  wf._n_sites = 8
  wf.initialize(seed=1)
  os.makedirs(directory, exist_ok=True)
  session_lib.Saver(wf.get_trainable_variables()).save(None, os.path.join(directory, 'model_prior_0_epochs'))
  return hp


def test_lower_state_checkpoint_mismatch_names_the_variable(tmp_path):
  from cgs_vmc_amd import run_excited_state_training as rx
  hp = _checkpoint(str(tmp_path / 'same'), 12)
  _checkpoint(str(tmp_path / 'other'), 20)
  wavefunctions.reset_name_scope()
  psi = wavefunctions.build_wavefunction(hp)
  data = rx.check_lower_state(psi, 8, str(tmp_path / 'same'))
  assert data['fully_connected_network/linear/w'].shape == (8, 12)
  with pytest.raises(ValueError, match=r'fully_connected_network/linear/w .*\(8, 20\)'):
    rx.check_lower_state(psi, 8, str(tmp_path / 'other'))
  with pytest.raises(ValueError, match='no checkpoint'):
    rx.check_lower_state(psi, 8, str(tmp_path / 'empty'))
  # another architecture altogether: the first variable the checkpoint does not hold is named
  wavefunctions.reset_name_scope()
  rbm = wavefunctions.build_wavefunction(utils.create_hparams(num_sites=8, wavefunction_type='rbm', fc_layer_size=12,
                                                              num_fc_layers=1))
  rbm._n_sites = 8
  first = rbm.get_trainable_variables()[0].name
  with pytest.raises(ValueError, match='no variable ' + first):
    rx.check_lower_state(rbm, 8, str(tmp_path / 'same'))


def test_excited_state_flag_table_extends_run_training():
  from cgs_vmc_amd import run_excited_state_training as rx, run_training
  names = [row[0] for row in rx.FLAG_TABLE]
  assert names == [row[0] for row in run_training.FLAG_TABLE] + ['lower_state_dir', 'overlap_penalty']
  assert dict((r[0], r[2]) for r in rx.FLAG_TABLE)['optimizer'] == 'PenalizedEnergyGradient'
  assert dict((r[0], r[2]) for r in run_training.FLAG_TABLE)['optimizer'] == 'ITSWO'
  with pytest.raises(ValueError, match='lower_state_dir'):
    rx.main(['--checkpoint_dir', 'unused', '--overlap_penalty', '1.0'])
  with pytest.raises(ValueError, match='overlap_penalty'):
    rx.main(['--checkpoint_dir', 'unused', '--lower_state_dir', 'unused'])


# ---- file round trips

def test_driver_file_round_trips(tmp_path):
  from cgs_vmc_amd import run_excited_state_training as rx, run_overlap_evaluation as ro
  result = {'fidelity': 0.0123456789012345678, 'fidelity_err': 0.00031, 'overlap_sign': -1.0,
            'alive_fraction': 0.984375, 'samples': np.zeros((2, 4))}
  path = ro.write_overlap(str(tmp_path), result)
  assert os.path.basename(path) == 'overlap.txt'
  back = ro.read_overlap(str(tmp_path))
  assert back['fidelity'] == result['fidelity'] and back['alive_fraction'] == result['alive_fraction']
  assert back['overlap_sign'] == -1.0 and back['fidelity_err'] == pytest.approx(result['fidelity_err'], rel=1e-5)
  values = [0.91, 0.5, 0.012345678]
  for v in values:
    assert os.path.basename(rx.write_overlap_metric(str(tmp_path), v)) == 'overlap_metrics.txt'
  assert rx.read_overlap_metrics(str(tmp_path)) == values
  assert [row[0] for row in ro.FLAG_TABLE] == ['checkpoint_dir', 'other_dir', 'output_dir', 'hparams']

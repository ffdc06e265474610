"""CPU: the pbdg ansatz's front end (ProjectedBDG, wavefunctions.py:876-928) -- registry, variable name and shape,
initialiser, odd-N refusal, checkpoint names -- and the fp64 oracle (tests/pbdg_oracle.py): sign convention,
exchange ratio and log-derivatives."""
import copy
import itertools
import os
import subprocess

import numpy as np
import pytest

from cgs_vmc_amd import session, tf_checkpoint, utils, wavefunctions
from oracle import vmc_oracle as vo
from tests import pbdg_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fresh():
  session.reset_default_graph()
  wavefunctions.reset_name_scope()


def _perm_sign(p):
  p = list(p)
  s = 1
  for i in range(len(p)):
    for j in range(i + 1, len(p)):
      if p[i] > p[j]:
        s = -s
  return s


def test_oracle_determinant_is_the_sorted_mask_determinant_by_brute_force():
  """det M by the Leibniz sum over the sorted boolean-mask order, against the oracle's sign and logit."""
  rng = np.random.default_rng(0)
  n_sites = 8
  theta = rng.uniform(-1, 1, n_sites * n_sites)
  f = theta.reshape(n_sites, n_sites)
  cfg = vo.random_configurations(n_sites, 12, np.random.RandomState(1))
  logit, sign = po.logit_sign(theta, cfg)
  for row, lg, sg in zip(cfg, logit, sign):
    up = [i for i in range(n_sites) if row[i] > 0]
    dn = [i for i in range(n_sites) if row[i] < 0]
    det = sum(_perm_sign(p) * np.prod([f[up[r], dn[p[r]]] for r in range(4)])
              for p in itertools.permutations(range(4)))
    assert np.sign(det) == sg and abs(np.log(abs(det)) - lg) < 1e-12


def test_oracle_exchange_ratio_matches_direct_determinants():
  rng = np.random.default_rng(2)
  n_sites = 12
  theta = rng.uniform(-1, 1, n_sites * n_sites)
  cfg = vo.random_configurations(n_sites, 400, np.random.RandomState(3))
  worst = 0.0
  for row in cfg:
    a = int(rng.choice(np.flatnonzero(row > 0)))
    b = int(rng.choice(np.flatnonzero(row < 0)))
    got = po.exchange_ratio(theta, row, a, b)
    ref = po.exchange_ratio_direct(theta, row, a, b)
    worst = max(worst, abs(got - ref) / max(abs(ref), 1e-300))
  assert worst < 1e-9, worst


def test_oracle_log_derivatives_match_finite_differences():
  rng = np.random.default_rng(4)
  n_sites = 8
  theta = rng.uniform(-1, 1, n_sites * n_sites)
  cfg = vo.random_configurations(n_sites, 3, np.random.RandomState(5))
  o = po.log_derivatives(theta, cfg)
  h = 1e-6
  for p in range(theta.size):
    d = np.zeros_like(theta)
    d[p] = h
    fd = (po.logit_sign(theta + d, cfg)[0] - po.logit_sign(theta - d, cfg)[0]) / (2 * h)
    np.testing.assert_allclose(o[:, p], fd, rtol=1e-5, atol=1e-7)
  assert (np.count_nonzero(o, axis=1) == (n_sites // 2) ** 2).all()


def test_oracle_singular_pairing_gives_zero_not_nan():
  theta = np.random.default_rng(6).uniform(-1, 1, 36).reshape(6, 6)
  theta[1] = 0.0                               # a zero row of F: every M holding up site 1 is singular
  cfg = vo.random_configurations(6, 40, np.random.RandomState(7))
  p = po.psi(theta.ravel(), cfg)
  both = cfg[:, 1] > 0
  assert both.any() and (p[both] == 0).all() and np.isfinite(p).all()


def test_oracle_update_norm_keeps_the_shift_without_positive_amplitudes():
  assert po.update_norm_shift(np.array([-1e12, -3.0]), 5.0) == 5.0
  assert po.update_norm_shift(np.array([-1e12, 1e12]), 5.0) == pytest.approx(5.0 + np.log(100.0))


def test_pbdg_class_names_shapes_and_init_bounds(monkeypatch):
  _fresh()
  monkeypatch.setenv('CGS_VMC_INIT_SEED', '3')
  hp = utils.create_hparams(wavefunction_type='pbdg', num_sites=16)
  wf = wavefunctions.build_wavefunction(hp)
  assert isinstance(wf, wavefunctions.ProjectedBDG)
  assert wavefunctions.WAVEFUNCTION_TYPES['pbdg'] is wavefunctions.ProjectedBDG
  assert wf._shapes() == (['projected_bdg/pairing_matrix'], [(1, 16, 16)])
  assert wf.num_params == 256
  assert wf._get_shift() == np.float32(-10.0)
  spec = wf._engine_spec()
  assert spec['ansatz'] == 'pbdg'
  dc = copy.deepcopy(wf)
  assert dc._shapes() == (['dc_projected_bdg/pairing_matrix'], [(1, 16, 16)])
  assert dc._engine_spec() == spec
  wf._n_sites = 16
  wf.initialize(11)
  theta = wf._get_theta()
  lim = np.sqrt(3.0 / 16)
  assert theta.shape == (256,) and np.abs(theta).max() <= lim and np.abs(theta).max() > 0.9 * lim
  assert abs(theta.mean()) < 0.05 and abs(theta.std() - lim / np.sqrt(3)) < 0.03


def test_pbdg_odd_sites_raise_value_error():
  _fresh()
  with pytest.raises(ValueError):
    wavefunctions.build_wavefunction(utils.create_hparams(wavefunction_type='pbdg', num_sites=15))
  with pytest.raises(ValueError):
    wavefunctions.ProjectedBDG(7)


def test_pbdg_checkpoint_names(tmp_path):
  """The trainable variable set of a checkpoint (B7): one pairing matrix, in both formats' names."""
  _fresh()
  wf = wavefunctions.ProjectedBDG(10)
  wf._n_sites = 10
  wf.initialize(1)
  variables = wf.get_trainable_variables()
  assert [v.name for v in variables] == ['projected_bdg/pairing_matrix']
  assert tuple(variables[0].shape) == (1, 10, 10)
  value = np.asarray(variables[0].eval())
  path = str(tmp_path / 'model')
  tf_checkpoint.write_bundle(path, {'projected_bdg/pairing_matrix': value.reshape(1, 10, 10)})
  back = tf_checkpoint.read_bundle(path)
  np.testing.assert_array_equal(back['projected_bdg/pairing_matrix'].ravel(), value.ravel())


def test_pbdg_planner_hostcheck_cases():
  """plan_pbdg_* under AddressSanitizer + UBSan (make hostcheck; its pbdg grid)."""
  src = open(os.path.join(ROOT, 'cgs_vmc_amd', 'csrc', 'hostcheck.cpp')).read()
  assert 'pbdg_grid' in src
  r = subprocess.run(['make', '-s', '-C', os.path.join(ROOT, 'cgs_vmc_amd', 'csrc'), 'hostcheck'],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr

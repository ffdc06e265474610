"""CPU: the fully_connected_nnb ansatz's front end (FullyConnectedNNB, wavefunctions.py:931-998) -- registry, variable
names, shapes and order, initialiser, refusals, no exponent shift, checkpoints -- and the fp64 oracle
(tests/nnb_oracle.py): determinant convention, log-derivatives, the bridge to pbdg."""
import copy
import itertools
import os
import subprocess

import numpy as np
import pytest

from cgs_vmc_amd import session, tf_checkpoint, utils, wavefunctions
from oracle import vmc_oracle as vo
from tests import nnb_oracle as no
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


def test_build_wavefunction_returns_the_nnb_class():
  _fresh()
  hp = utils.create_hparams(wavefunction_type='fully_connected_nnb', num_sites=16, num_fc_layers=2, fc_layer_size=32)
  wf = wavefunctions.build_wavefunction(hp)
  assert isinstance(wf, wavefunctions.FullyConnectedNNB)
  assert wavefunctions.WAVEFUNCTION_TYPES['fully_connected_nnb'] is wavefunctions.FullyConnectedNNB
  assert wf._engine_spec() == dict(ansatz='fully_connected_nnb', num_layers=2, layer_size=32, nonlinearity='relu',
                                   output_activation='exp')


def test_nnb_variable_names_shapes_order_and_count():
  _fresh()
  n, l, h = 16, 3, 24
  wf = wavefunctions.FullyConnectedNNB(n, l, [h] * l)
  names, shapes = wf._shapes()
  u = 'fully_connected_nnb'
  assert names == [u + '/linear/w', u + '/linear/b', u + '/linear_1/w', u + '/linear_1/b', u + '/linear_2/w',
                   u + '/linear_2/b', u + '/linear_3/w', u + '/linear_3/b']
  assert shapes == [(n, h), (h,), (h, h), (h,), (h, h), (h,), (h, n * n), (n * n,)]
  p = n * h + h + (l - 1) * (h * h + h) + h * n * n + n * n
  assert wf.num_params == p == no.num_params(n, l, h)
  dc = copy.deepcopy(wf)
  assert dc._shapes()[0][0] == 'dc_fully_connected_nnb/linear/w' and dc._shapes()[1] == shapes
  assert dc._engine_spec() == wf._engine_spec()


def test_nnb_initialiser_statistics():
  _fresh()
  n, l, h = 16, 2, 64
  wf = wavefunctions.FullyConnectedNNB(n, l, [h, h])
  wf.initialize(5)
  theta = wf._get_theta()
  assert theta.shape == (wf.num_params,)
  off, fan_in = 0, n
  for width in (h, h, n * n):
    w = theta[off:off + fan_in * width]; off += fan_in * width
    b = theta[off:off + width]; off += width
    sigma = 1 / np.sqrt(fan_in)
    assert np.abs(w).max() <= 2 * sigma * (1 + 1e-6) and np.abs(w).max() > 1.8 * sigma
    # a normal truncated at 2 sigma has standard deviation 0.8796 sigma
    assert abs(w.std() - 0.8796 * sigma) < 0.05 * sigma and abs(w.mean()) < 0.05 * sigma
    assert (b == 0).all()
    fan_in = width


def test_nnb_refusals():
  _fresh()
  with pytest.raises(ValueError):
    wavefunctions.FullyConnectedNNB(15, 1, [8])
  with pytest.raises(ValueError):
    wavefunctions.build_wavefunction(utils.create_hparams(wavefunction_type='fully_connected_nnb', num_sites=9))
  with pytest.raises(NotImplementedError):
    wavefunctions.FullyConnectedNNB(16, 0, [])
  with pytest.raises(NotImplementedError):
    wavefunctions.FullyConnectedNNB(16, 2, [8, 16])
  with pytest.raises(NotImplementedError):
    wavefunctions.FullyConnectedNNB(258, 1, [8])
  with pytest.raises(NotImplementedError):
    wavefunctions.FullyConnectedNNB(16, 1, [1024])


def test_nnb_has_no_exponent_shift():
  _fresh()
  wf = wavefunctions.FullyConnectedNNB(8, 1, [4])
  assert wf._exp_norm_shift is None
  assert wf.normalize_batch(object()) is None and wf.update_norm(object()) is None


def test_nnb_checkpoint_round_trip_in_both_formats(tmp_path):
  _fresh()
  wf = wavefunctions.FullyConnectedNNB(8, 2, [6, 6])
  wf.initialize(1)
  variables = wf.get_trainable_variables()
  values = {v.name: np.asarray(v.eval()).reshape(v.shape) for v in variables}
  assert list(values) == wf._shapes()[0]
  path = str(tmp_path / 'model')
  tf_checkpoint.write_bundle(path, values)
  back = tf_checkpoint.read_bundle(path)
  np.savez(str(tmp_path / 'model.npz'), **values)
  npz = np.load(str(tmp_path / 'model.npz'))
  _fresh()
  twin = wavefunctions.FullyConnectedNNB(8, 2, [6, 6])
  twin._n_sites = 8
  for source in (back, npz):
    for v in twin.get_trainable_variables():
      v.load(np.zeros(v.shape, np.float32))
    for v in twin.get_trainable_variables():
      assert tuple(source[v.name].shape) == tuple(v.shape)
      v.load(source[v.name])
    np.testing.assert_array_equal(twin._get_theta(), wf._get_theta())


def test_oracle_determinant_is_the_sorted_mask_determinant_by_brute_force():
  n, l, h = 8, 2, 16                 # (zero output biases: F(x) has rank <= the active units, so h >= n/2)
  theta = no.default_theta(n, l, h, 0)
  cfg = vo.random_configurations(n, 10, np.random.RandomState(1))
  logit, sign = no.logit_sign(theta, cfg, l, h)
  _, out = no.forward(theta, cfg, l, h)
  for row, o, lg, sg in zip(cfg, out, logit, sign):
    f = o.reshape(n, n)
    up = [i for i in range(n) if row[i] > 0]
    dn = [i for i in range(n) if row[i] < 0]
    det = sum(_perm_sign(p) * np.prod([f[up[r], dn[p[r]]] for r in range(4)])
              for p in itertools.permutations(range(4)))
    assert np.sign(det) == sg and abs(np.log(abs(det)) - lg) < 1e-10


def test_oracle_log_derivatives_match_central_differences_over_every_parameter():
  n, l, h = 6, 2, 4
  rng = np.random.default_rng(2)
  theta = no.default_theta(n, l, h, 3).astype(np.float64)
  theta += 0.1 * rng.standard_normal(theta.size)         # nonzero biases, pre-activations away from the relu kink
  cfg = vo.random_configurations(n, 3, np.random.RandomState(4))
  o = no.log_derivatives(theta, cfg, l, h)
  assert o.shape == (3, no.num_params(n, l, h))
  step = 1e-6
  for p in range(theta.size):
    d = np.zeros_like(theta)
    d[p] = step
    fd = (no.logit_sign(theta + d, cfg, l, h)[0] - no.logit_sign(theta - d, cfg, l, h)[0]) / (2 * step)
    np.testing.assert_allclose(o[:, p], fd, rtol=2e-5, atol=2e-7)


def test_oracle_bridge_to_pbdg():
  """W_out = 0 and b_out = F.ravel(): the backflow state is pbdg's determinant of that F."""
  n, l, h = 8, 2, 6
  theta = no.default_theta(n, l, h, 5).astype(np.float64)
  f = np.random.default_rng(6).uniform(-1, 1, n * n)
  ow, ob = no.offsets(n, l, h)
  theta[ow:ob] = 0.0
  theta[ob:] = f
  cfg = vo.random_configurations(n, 20, np.random.RandomState(7))
  lg, sg = no.logit_sign(theta, cfg, l, h)
  ref_l, ref_s = po.logit_sign(f, cfg)
  np.testing.assert_allclose(lg, ref_l, rtol=0, atol=1e-12)
  np.testing.assert_array_equal(sg, ref_s)
  o = no.log_derivatives(theta, cfg, l, h)
  np.testing.assert_allclose(o[:, ob:], po.log_derivatives(f, cfg), rtol=1e-12, atol=1e-14)


def test_nnb_planner_hostcheck_cases():
  """plan_nnb_* under AddressSanitizer + UBSan (make hostcheck; its nnb grid)."""
  src = open(os.path.join(ROOT, 'cgs_vmc_amd', 'csrc', 'hostcheck.cpp')).read()
  assert 'nnb_grid' in src
  r = subprocess.run(['make', '-s', '-C', os.path.join(ROOT, 'cgs_vmc_amd', 'csrc'), 'hostcheck'],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize('n_sites', [130, 160])
def test_large_nnb_local_energy_bound_is_measured_and_sharp(n_sites):
  """The local-energy bound of tests/test_gpu_det_large.py's nnb rows: the stored c is the float32 emulation's
  (no.exchange_terms: trunk, pairing layer, elimination and logit difference in float32), the fp64 terms sum to
  no.local_energy, and one term of the wrong sign moves E_loc by more than the bound for at least 90 % of the terms of
  every row."""
  from tests import det_large_cases as dc
  from tests import pbdg_oracle as po
  l, h = dc.NNB_LAYERS, dc.NNB_UNITS
  theta, cfg, bonds, jx, jz = dc.nnb_inputs(n_sites)
  eps = np.finfo(np.float32).eps
  terms = no.exchange_terms(theta, cfg, bonds, jx, l, h)
  diag = po.diagonal_energy(cfg, bonds, jz)
  np.testing.assert_allclose(diag + terms.sum(1), no.local_energy(theta, cfg, bonds, jx, jz, l, h), rtol=1e-9)
  t32 = no.exchange_terms(theta, cfg, bonds, jx, l, h, np.float32)
  e32 = po.diagonal_energy(cfg, bonds, jz, np.float32) + t32.sum(1, dtype=np.float32)
  ratio = (np.abs(e32 - (diag + terms.sum(1))) / (eps * np.abs(terms).sum(1))).max()
  stored = dc.EMULATED_NNB_ELOC_RATIO[n_sites]
  assert stored / 2 <= ratio <= 2 * stored, (ratio, stored)
  bound = dc.nnb_eloc_bound(n_sites, terms, diag)
  shares = [(2 * np.abs(t[t != 0]) > b).mean() for t, b in zip(terms, bound)]
  print('nnb N = %d: err / (eps32 sum|terms|) %.3g (stored %.3g); share of terms whose flip exceeds the bound: %s'
        % (n_sites, ratio, stored, np.round(shares, 3)))
  assert min(shares) >= 0.9

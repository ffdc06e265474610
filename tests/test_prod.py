"""CPU side of the 'prod' composite (ProductOfWavefunctions, wavefunctions.py:107-161, 1178-1194): build_wavefunction, the
variables and names, the deep copy, the refusals that still stand, and the fp64 product oracle against brute force."""
import copy

import numpy as np
import pytest

from cgs_vmc_amd import session, utils, wavefunctions
from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo
from tests import prod_oracle as pro


@pytest.fixture(autouse=True)
def _fresh_graph():
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  yield
  session.reset_default_graph(); wavefunctions.reset_name_scope()


def _hparams(types=('pbdg', 'fully_connected'), acts=('exp', 'exp'), **kw):
  return utils.create_hparams(wavefunction_type='prod', composite_wavefunction_types=list(types),
                              composite_output_activations=list(acts), num_sites=16, **kw)


def _connect(wf, n=16):
  """What _bind does to the factors' shapes, without an engine."""
  for sub in wf._sub_wavefunctions:
    sub._n_sites = n
    sub.initialize(0)


def test_build_wavefunction_returns_the_product_with_the_reference_name():
  wf = wavefunctions.build_wavefunction(_hparams(num_fc_layers=2, fc_layer_size=32))
  assert isinstance(wf, wavefunctions.ProductOfWavefunctions)
  a, b = wf._sub_wavefunctions
  assert isinstance(a, wavefunctions.ProjectedBDG) and type(b) is wavefunctions.FullyConnectedNetwork
  assert wf._unique_name == '_times_'.join([b._unique_name, a._unique_name]) == 'fully_connected_network_times_projected_bdg'
  assert wf._exp_norm_shift is None and wf.update_norm(None) is None and wf.normalize_batch(None) is None
  _connect(wf)
  names = [v.name for v in wf.get_trainable_variables()]
  assert names == [v.name for v in a.get_trainable_variables()] + [v.name for v in b.get_trainable_variables()]
  assert names[0] == 'projected_bdg/pairing_matrix' and names[1] == 'fully_connected_network/linear/w'
  assert all(n.split('/')[0] in (a._unique_name, b._unique_name) for n in names)


def test_deepcopy_has_independent_values_and_transfer_covers_both_factors():
  wf = wavefunctions.build_wavefunction(_hparams(num_fc_layers=1, fc_layer_size=8))
  _connect(wf)
  twin = copy.deepcopy(wf)
  assert isinstance(twin, wavefunctions.ProductOfWavefunctions) and twin._unique_name == 'dc_' + wf._unique_name
  assert [s._unique_name for s in twin._sub_wavefunctions] == ['dc_' + s._unique_name for s in wf._sub_wavefunctions]
  for sub in twin._sub_wavefunctions:
    sub._n_sites = 16
    sub._set_theta(np.zeros(sub.num_params, np.float32))
  src, dst = wf.get_trainable_variables(), twin.get_trainable_variables()
  assert len(src) == len(dst) == 5 and all(np.all(v.eval() == 0) for v in dst)
  before = [v.eval().copy() for v in src]
  session.Session().run(wavefunctions.module_transfer_ops(wf, twin))
  for s, d, b in zip(src, dst, before):
    np.testing.assert_array_equal(d.eval(), s.eval())
    np.testing.assert_array_equal(s.eval(), b)
  dst[0].load(np.ones(dst[0].shape, np.float32))              # the twin's values are its own
  np.testing.assert_array_equal(src[0].eval(), before[0])


def test_two_factors_of_one_type_get_distinct_scopes():
  wf = wavefunctions.build_wavefunction(_hparams(types=('fully_connected', 'fully_connected'), num_fc_layers=1,
                                                 fc_layer_size=4))
  a, b = wf._sub_wavefunctions
  assert a._unique_name == 'fully_connected_network' and b._unique_name == 'fully_connected_network_1'
  assert wf._unique_name == 'fully_connected_network_1_times_fully_connected_network'
  _connect(wf)
  names = [v.name for v in wf.get_trainable_variables()]
  assert len(set(names)) == len(names) == 8


def test_scalar_factor_and_from_hparams_are_refused():
  wf = wavefunctions.FullyConnectedNetwork(1, 4)
  with pytest.raises(NotImplementedError):
    wf * 2.0
  with pytest.raises(NotImplementedError):
    wf * session.Tensor(lambda: 2.0, 'two')
  prod = wf * wavefunctions.ProjectedBDG(16)
  with pytest.raises(ValueError, match='Hparams initialization is not supported for product.'):
    prod.from_hparams(_hparams())
  with pytest.raises(ValueError, match='Hparams initialization is not supported for product.'):
    wavefunctions.ProductOfWavefunctions.from_hparams(_hparams())
  with pytest.raises(NotImplementedError):
    prod * wf                                                   # a product of products


def test_refusals_that_still_stand():
  for kind in ('sum', 'diff'):
    with pytest.raises(NotImplementedError, match='composite wavefunctions are outside the MI355X hot path'):
      wavefunctions.build_wavefunction(utils.create_hparams(
          wavefunction_type=kind, composite_wavefunction_types=['pbdg', 'fully_connected'],
          composite_output_activations=['exp', 'exp'], num_sites=16))
  a, b = wavefunctions.FullyConnectedNetwork(1, 4), wavefunctions.FullyConnectedNetwork(1, 4)
  with pytest.raises(NotImplementedError):
    a + b
  with pytest.raises(NotImplementedError):
    a - b
  with pytest.raises(ValueError):
    wavefunctions.build_wavefunction(_hparams(types=('pbdg', 'no_such_type')))
  with pytest.raises(NotImplementedError):
    wavefunctions.build_wavefunction(_hparams(types=('mps', 'fully_connected')))


def test_bind_refuses_a_distributed_run_and_a_non_exp_factor(monkeypatch):
  """_bind refuses before it asks for an engine, so neither case needs a GPU."""
  from cgs_vmc_amd import parallel
  wf = wavefunctions.build_wavefunction(_hparams(num_fc_layers=1, fc_layer_size=8))
  monkeypatch.setattr(parallel, 'is_distributed', lambda: True)
  with pytest.raises(NotImplementedError, match='prod'):
    wf._bind(None)
  monkeypatch.setattr(parallel, 'is_distributed', lambda: False)
  tanh = wavefunctions.build_wavefunction(_hparams(acts=('exp', 'tanh'), num_fc_layers=1, fc_layer_size=8))
  with pytest.raises(NotImplementedError, match='prod: a dense factor needs the exp output activation'):
    tanh._bind(None)


# ---- the oracle against brute force on 4 sites: an explicit fp64 state vector psi_a psi_b over all 16 configurations
def _all_configs(n):
  return np.array([[1.0 if (w >> i) & 1 else -1.0 for i in range(n)] for w in range(1 << n)], np.float32)


def _brute(vec, words, bonds, jx, jz, n):
  """E_loc of an explicit vector over the basis, by building H as a dense matrix."""
  dim = 1 << n
  h = np.zeros((dim, dim))
  for w in range(dim):
    for (i, j) in bonds:
      si, sj = (w >> i) & 1, (w >> j) & 1
      h[w, w] += 0.25 * jz * (1 if si == sj else -1)
      if si != sj:
        h[w ^ (1 << i) ^ (1 << j), w] += 0.5 * jx
  return (h.T @ vec)[words] / vec[words]


def test_product_oracle_matches_brute_force_on_four_sites():
  n, h, L, jx, jz, beta = 4, 3, 1, 0.7, 1.3, 0.05
  rng = np.random.default_rng(5)
  bonds = vo.chain_bonds(n)
  th_a, th_b = vo.init_params(n, h, L, rng), vo.rbm_init_params(n, h, 0, rng)
  tw_a, tw_b = th_a + 0.1 * rng.standard_normal(th_a.size), th_b + 0.1 * rng.standard_normal(th_b.size)
  prod = pro.Product(pro.fc_factor(th_a, h, L, 0.0), pro.rbm_factor(th_b, h, 0, 0.0))
  omega = pro.Product(pro.fc_factor(tw_a, h, L, 0.0), pro.rbm_factor(tw_b, h, 0, 0.0))
  basis = _all_configs(n)
  words = np.arange(1 << n)
  vec = np.asarray(prod.a.psi(basis), np.float64) * np.asarray(prod.b.psi(basis), np.float64)
  vec_w = np.asarray(omega.a.psi(basis), np.float64) * np.asarray(omega.b.psi(basis), np.float64)
  np.testing.assert_allclose(prod.psi(basis), vec, rtol=1e-12)
  e_ref = _brute(vec, words, bonds, jx, jz, n)
  np.testing.assert_allclose(prod.local_energy(basis, bonds, jx, jz), e_ref, rtol=1e-12, atol=1e-12)
  # O by central differences of ln|psi_a psi_b| is too coarse for 1e-12: the log-derivative of a product is the
  # concatenation of the factors' own, checked against d ln(vec) through the factors' analytic gradients summed
  o = prod.log_grads(basis)
  assert o.shape == (1 << n, th_a.size + th_b.size)
  np.testing.assert_allclose(o[:, :th_a.size], prod.a.log_grads(basis), rtol=1e-12)
  np.testing.assert_allclose(o[:, th_a.size:], prod.b.log_grads(basis), rtol=1e-12)
  eps = 1e-6
  for k in (0, th_a.size - 1, th_a.size, th_a.size + th_b.size - 1):
    tp = prod.theta.copy(); tp[k] += eps
    tm = prod.theta.copy(); tm[k] -= eps
    f = lambda t: np.log(np.abs(np.asarray(pro.fc_factor(t[:th_a.size], h, L, 0.0).psi(basis), np.float64) *
                                np.asarray(pro.rbm_factor(t[th_a.size:], h, 0, 0.0).psi(basis), np.float64)))
    np.testing.assert_allclose(o[:, k], (f(tp) - f(tm)) / (2 * eps), rtol=1e-6, atol=1e-8)
  # both optimizers' gradients from the explicit vectors
  acc = vo.Accumulators(prod.num_params, np.float64)
  pro.energy_gradient_accumulate(acc, prod, basis, bonds, jx, jz)
  g_ref = (e_ref[:, None] * o).sum(0) - e_ref.mean() * o.sum(0)      # (mean_tensor: one count per accumulate call)
  np.testing.assert_allclose(vo.energy_gradient(acc), g_ref, rtol=1e-12, atol=1e-13)
  acc = vo.Accumulators(prod.num_params, np.float64)
  pro.log_overlap_accumulate(acc, prod, omega, basis, bonds, jx, jz, beta)
  ew = _brute(vec_w, words, bonds, jx, jz, n)
  ratio = vec_w / vec * (1 - beta * ew)
  g_ref = o.sum(0) - (ratio[:, None] * o).sum(0) / ratio.mean()
  np.testing.assert_allclose(vo.log_overlap_gradient(acc), g_ref, rtol=1e-12, atol=1e-13)


def test_product_oracle_with_signed_factors():
  n = 4
  top, bot, length = eo.lin_tables(n)
  cfg = eo.sz0_configurations(n)
  vec = np.random.default_rng(1).standard_normal(length)
  th = np.random.default_rng(2).uniform(-1, 1, n * n)
  prod = pro.Product(pro.pbdg_factor(th, 0.0), pro.edvec_factor(vec, top, bot))
  from tests import pbdg_oracle as po
  np.testing.assert_allclose(prod.psi(cfg), po.psi(th, cfg, 0.0) * vec[eo.index(cfg, top, bot)], rtol=1e-12)
  assert (np.sign(prod.psi(cfg)) == np.sign(po.psi(th, cfg, 0.0)) * np.sign(vec[eo.index(cfg, top, bot)])).all()


# ---- the inputs of tests/test_gpu_prod_shapes.py (tests/prod_shape_cases.py): the conditions its checks lean on, proved
# on the oracle alone
from tests import prod_shape_cases as psc     # noqa: E402


@pytest.mark.parametrize('cid', psc.IDS)
def test_shape_case_replay_stays_inside_the_caps(cid):
  """Banded verdicts over the whole replay: at most 2 chains (S5: none, so mc_steps' count is compared exactly);
  acceptance share in [0.2, 0.8] on S1-S5, so k_prod_accept's patched-spin path runs both ways; S6, one chain: at least
  one accept and one reject."""
  c, r = psc.CASES[cid], psc.replay(cid)
  assert c['steps'] == {'S4': 40, 'S5': 20}.get(cid, 3 * c['n'])
  print('%s: share %.3f, accepted %d of %d, banded chains %d' % (cid, r.share, r.accepted, r.accepts.size, r.band.sum()))
  assert r.band.sum() <= (0 if cid == 'S5' else 2)
  assert r.accepts.shape == (c['steps'], c['b_chains']) and (r.configs.sum(1) == 0).all()
  if cid == 'S6':
    assert r.accepts.any() and not r.accepts.all()
  else:
    assert 0.2 <= r.share <= 0.8
  assert (r.configs != psc.start(cid)).any()


def test_shape_case_evaluation_replay_has_no_banded_verdict():
  eq, samples = psc.eval_replay()
  assert not eq.band.any() and not any(s.band.any() for s in samples)
  assert all(0 < s.accepted < s.accepts.size for s in samples)


@pytest.mark.parametrize('cid', psc.IDS)
def test_shape_case_inputs(cid):
  """The bond list is irregular (N + 5 bonds, some i > j, one jx = 0, one jx < 0), the offsets and tails are the ones
  the table names, and the pbdg logit bound 64 (N/2) eps32 kappa stays below 0.5 on every test row, so every sign is
  checked."""
  c = psc.CASES[cid]
  bonds, jx, jz = psc.bonds(cid)
  n = c['n']
  assert len(bonds) == n + 5 and all(i != j and 0 <= i < n and 0 <= j < n for i, j in bonds)
  assert any(i > j for i, j in bonds) and any(i < j for i, j in bonds) and any(abs(i - j) > 2 for i, j in bonds)
  assert (jx == 0).sum() == 1 and (jx < 0).sum() == 1 and jx[(jx != 0) & (jx > 0)].min() >= 0.3 and jx.max() <= 1.7
  assert jz.min() >= -1.0 and jz.max() <= 1.5
  prod = psc.product_of(cid)
  rows = psc.compared_rows(cid)
  assert (rows.sum(1) == 0).all()
  bound = psc.pbdg_logit_bound(prod, rows)
  print('%s: largest pbdg logit bound %.3g over %d rows' % (cid, bound.max(), len(rows)))
  assert bound.max() < 0.5
  assert np.isfinite(np.log(np.abs(prod.psi(rows)))).all()
  if psc.signed(cid) and c['b_chains'] > 4:
    ref = prod.psi(psc.start(cid))
    assert (ref > 0).any() and (ref < 0).any()        # both signs among the start chains
  for th in psc.thetas(cid):
    assert th.dtype == np.float32
  if cid == 'S4':
    assert (n + 3) // 4 == 65 and n % 4 == 2         # block 64: lane 0's second trip, two valid sites
  if cid == 'S5':
    assert c['b_chains'] > 1024 and c['b_chains'] % 4 == 1


def test_shape_case_sampler_proposals_reach_the_last_philox_block():
  """S4: over the replay some proposal names a site of Philox block 64 (sites 256, 257), and some accepted move has
  changed a spin there before a later proposal -- the second trip of k_prod_accept's loop with patched spins decides."""
  cid = 'S4'
  prod, cur = psc.product_of(cid), psc.start(cid)
  hit = 0
  for k in range(psc.CASES[cid]['steps']):
    i_up, i_dn, u = psc.proposals(cid, cur, k)
    hit += int(((i_up >= 256) | (i_dn >= 256)).sum())
    cur, _, _ = pro.mc_step(prod, cur, i_up, i_dn, u)
  assert hit >= 1


@pytest.mark.parametrize('name', sorted(psc.SCRIPTS))
def test_shape_case_injected_scripts_hold_every_group(name):
  """At least two chains start on psi = 0 and leave on their first non-zero candidate, at least two candidates land on
  a zero and are rejected, at least two proposals name sites with the wrong spins; no verdict is banded."""
  s = psc.SCRIPTS[name]()
  print('%s: zero starts %d (left on a non-zero candidate %d), zero candidates %d, bad proposals %d' % (
      name, s.zero_start, s.first_nonzero_accepts, s.zero_cand, s.bad))
  assert s.zero_start >= 2 and s.first_nonzero_accepts >= 2 and s.zero_cand >= 2 and s.bad >= 2
  assert not s.band.any()
  assert (s.prod.psi(s.start) == 0).sum() >= 2
  for after in s.after:
    assert (after.sum(1) == 0).all()
  before = [s.start] + s.after[:-1]
  for cur, new, mask, bad in zip(before, s.after, s.masks, s.bads):       # a bad proposal: mask false, the chain stays
    assert not mask[bad].any() and (new[bad] == cur[bad]).all()
    assert ((new != cur).sum(1) == 2 * mask).all()
  assert s.bads[2].sum() >= 5 and not any(b.any() for k, b in enumerate(s.bads) if k != 2)


def test_shape_case_zero_supervisor_entries_sit_under_two_chains():
  top, bot, _ = eo.lin_tables(psc.CASES['S3']['n'])
  idx = eo.index(psc.start('S3'), top, bot)
  assert len(set(idx[:2].tolist())) == 2 and not np.isin(idx[2:], idx[:2]).any()


@pytest.mark.parametrize('cid', ['S1', 'S2', 'S3'])
def test_shape_case_supervisor_gives_ratios_of_both_signs(cid):
  _, e_w, ratio, _ = psc.itswo_reference(cid)
  assert np.isfinite(ratio).all() and np.isfinite(e_w).all() and (ratio > 0).any() and (ratio < 0).any()

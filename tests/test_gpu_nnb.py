"""GPU parity of the fully_connected_nnb ansatz -- FullyConnectedNNB (wavefunctions.py:931-998) on csrc/nnb.hip --
through the C ABI and the training front end, against the fp64 oracle (tests/nnb_oracle.py): amplitudes, the bridge to
pbdg, the singular case, local energies and both accumulators, the sampler, exact <H> by enumeration, sharded chains,
run_training / run_energy_evaluation and the refusals."""
import os

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import gnn_oracle as go
from tests import nnb_oracle as no
from tests import pbdg_oracle as po

pytestmark = pytest.mark.gpu

EPS32 = np.finfo(np.float32).eps


def _engine(n, b, l, h, **kw):
  from cgs_vmc_amd.engine import VmcEngine
  kw.setdefault('seed', 2024)
  return VmcEngine(n, b, l, h, ansatz='fully_connected_nnb', **kw)


@pytest.mark.parametrize('case', ['4x4', '6x6', '10x10'])
def test_nnb_amplitudes_match_the_fp64_oracle(case):
  """Signs equal and |logit - oracle| <= 64 n eps32 kappa(M) on every row (no row left out), seeded default
  initialisation; the chains' cache equals vmc_amplitude on the same rows bit for bit."""
  n, l, h, b = {'4x4': (16, 2, 32, 64), '6x6': (36, 2, 64, 48), '10x10': (100, 3, 256, 24)}[case]
  theta = no.default_theta(n, l, h, 1)
  cfg = vo.random_configurations(n, b, np.random.RandomState(2))
  eng = _engine(n, b, l, h)
  assert eng.kernel_path() == 8 and eng.num_params == no.num_params(n, l, h)
  eng.set_params(theta)
  eng.set_configs(cfg)
  logit, psi = eng.amplitude(cfg)
  ref_l, ref_s = no.logit_sign(theta, cfg, l, h)
  kappa = no.condition_numbers(theta, cfg, l, h)
  bound = 64 * (n // 2) * EPS32 * kappa
  err = np.abs(logit.astype(np.float64) - ref_l)
  print('nnb %s: max |dlogit| %.3g, max of err / (n eps32 kappa) %.3g, max kappa %.3g'
        % (case, err.max(), (err / ((n // 2) * EPS32 * kappa)).max(), kappa.max()))
  assert (err <= bound).all(), (err.max(), bound[err.argmax()])
  sign = np.where(np.signbit(psi), -1.0, 1.0)
  np.testing.assert_array_equal(sign, ref_s)
  with np.errstate(over='ignore'):
    np.testing.assert_allclose(np.abs(psi), np.exp(logit.astype(np.float64)).astype(np.float32), rtol=1e-5, atol=1e-37)
  logit_c, psi_c = eng.amplitude()
  np.testing.assert_array_equal(logit_c, logit)
  np.testing.assert_array_equal(psi_c, psi)
  assert eng.get_shift() == 0.0
  eng.set_shift(-10.0)
  eng.update_norm()
  assert eng.get_shift() == 0.0
  eng.close()


def _bridge_theta(n, l, h, f, seed):
  theta = no.default_theta(n, l, h, seed)
  ow, ob = no.offsets(n, l, h)
  theta[ow:ob] = 0.0
  theta[ob:] = f
  return theta, ob


def test_nnb_with_a_constant_pairing_layer_is_pbdg():
  """W_out = 0, b_out = F: amplitudes, local energies and the b_out block of the gradient sums equal a pbdg ctx."""
  from cgs_vmc_amd.engine import VmcEngine
  n, l, h, b = 16, 2, 32, 64
  f = np.random.default_rng(3).uniform(-np.sqrt(3.0 / n), np.sqrt(3.0 / n), n * n).astype(np.float32)
  theta, ob = _bridge_theta(n, l, h, f, 4)
  bonds = vo.torus_bonds(4, 4)
  cfg = vo.random_configurations(n, b, np.random.RandomState(5))
  eng = _engine(n, b, l, h)
  ref = VmcEngine(n, b, 1, 1, ansatz='pbdg', seed=2024)
  ref.set_shift(0.0)
  for e, t in ((eng, theta), (ref, f)):
    e.set_params(t); e.set_configs(cfg); e.set_bonds(bonds, 1.0, 1.0)
  (lg, ps), (lr, pr) = eng.amplitude(), ref.amplitude()
  kappa = po.condition_numbers(f, cfg)
  assert (np.abs(lg.astype(np.float64) - lr) <= 64 * (n // 2) * EPS32 * kappa).all()
  np.testing.assert_array_equal(np.sign(ps), np.sign(pr))
  e1, e2 = eng.local_energy()[0], ref.local_energy()[0]
  np.testing.assert_allclose(e1, e2, rtol=2e-3, atol=2e-3 * np.abs(e2).mean())
  for e in (eng, ref):
    e.reset_accumulators()
    e.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  a, r = eng.get_accumulators(), ref.get_accumulators()
  p = theta.size
  for got, want in ((a[ob:p], r[:n * n]), (a[p + ob:2 * p], r[n * n:2 * n * n])):
    assert np.abs(got - want).max() < 2e-3 * np.abs(want).max() + 1e-4
  eng.close(); ref.close()


def test_nnb_singular_pairing_gives_zero_never_nan():
  n, l, h, b = 12, 1, 16, 40
  f = np.random.default_rng(6).uniform(-0.5, 0.5, (n, n)).astype(np.float32)
  f[1] = 0.0                                             # a zero row of F: singular wherever site 1 is up
  theta, _ = _bridge_theta(n, l, h, f.ravel(), 7)
  cfg = vo.random_configurations(n, b, np.random.RandomState(8))
  eng = _engine(n, b, l, h)
  eng.set_params(theta)
  logit, psi = eng.amplitude(cfg)
  up1 = cfg[:, 1] > 0
  assert up1.any() and (psi[up1] == 0).all() and np.isneginf(logit[up1]).all()
  assert not np.isnan(psi).any() and not np.isnan(logit).any() and np.isfinite(logit[~up1]).all()
  # chains with site 1 down: some connected configurations are singular (ratio 0), no local energy is NaN
  chains = np.resize(cfg[~up1], (b, n)).astype(np.float32)
  bonds = go.triangular_bonds(3, 4)
  eng.set_configs(chains); eng.set_bonds(bonds, 1.0, 1.0)
  eloc = eng.local_energy()[0]
  ref = no.local_energy(theta, chains, bonds, 1.0, 1.0, l, h)
  assert np.isfinite(eloc).all()
  np.testing.assert_allclose(eloc, ref, rtol=2e-3, atol=2e-3 * np.abs(ref).mean())
  eng.close()


def _acc_close(got, acc, p):
  # the tolerance of tests/test_gpu_pbdg.py: fp32 inverses (kappa eps32 ~ 1e-4 per entry) summed over the batch
  for g, r in ((got[:p], acc.g1_total), (got[p:2 * p], acc.g2_total)):
    tol = 2e-3 * np.abs(r).max() + 1e-4
    assert np.abs(g - r).max() < tol, (np.abs(g - r).max(), tol)


def test_nnb_local_energies_and_accumulators(monkeypatch):
  """Triangular 6 x 6 cluster with jx = +1, both optimizers' accumulators (ITSWO against a perturbed supervisor, so that
  some ratios are negative); row blocks of 100 rows, so that several blocks run; two runs give identical bits."""
  monkeypatch.setenv('CGS_VMC_NNB_BLOCK_ROWS', '100')
  n, l, h, b = 36, 2, 64, 64
  bonds = go.triangular_bonds(6, 6)
  theta = no.default_theta(n, l, h, 9)
  cfg = vo.random_configurations(n, b, np.random.RandomState(10))
  theta_w = (theta + 0.05 * np.random.default_rng(11).standard_normal(theta.size) / np.sqrt(h)).astype(np.float32)
  p = theta.size
  runs = []
  for _ in range(2):
    eng = _engine(n, b, l, h)
    eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, 1.0, 1.0)
    eloc = eng.local_energy()[0]
    eng.reset_accumulators()
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    res_e = eng.get_accumulators()
    eng.transfer_params()
    eng.set_params(theta_w, _hip.VMC_OMEGA)
    eng.reset_accumulators()
    eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.05)
    res_o = eng.get_accumulators()
    runs.append((eloc, res_e, res_o))
    eng.close()
  for x, y in zip(runs[0], runs[1]):
    np.testing.assert_array_equal(x, y)
  eloc, res_e, res_o = runs[0]
  ref = no.local_energy(theta, cfg, bonds, 1.0, 1.0, l, h)
  np.testing.assert_allclose(eloc, ref, rtol=2e-3, atol=2e-3 * np.abs(ref).mean())
  acc = vo.Accumulators(p, np.float64)
  no.energy_gradient_accumulate(acc, theta, cfg, bonds, 1.0, 1.0, l, h)
  _acc_close(res_e, acc, p)
  assert abs(res_e[2 * p] - acc.e_total) < 2e-3 * max(1, abs(acc.e_total))
  acc = vo.Accumulators(p, np.float64)
  _, ratio = no.log_overlap_accumulate(acc, theta, theta_w, cfg, bonds, 1.0, 1.0, 0.05, l, h)
  assert (ratio < 0).any()
  _acc_close(res_o, acc, p)
  assert abs(res_o[2 * p + 2] - acc.r_total) < 2e-3 * max(1, np.abs(ratio).sum())


def test_nnb_sampler_injected_replayed_and_cached():
  n, l, h, b = 16, 2, 32, 64
  theta = no.default_theta(n, l, h, 12)
  amp = no.amp_fn(theta, l, h)
  cfg = vo.random_configurations(n, b, np.random.RandomState(13))
  eng = _engine(n, b, l, h)
  eng.set_params(theta); eng.set_configs(cfg)
  rng = np.random.default_rng(14)
  i_up = np.array([rng.choice(np.flatnonzero(r > 0)) for r in cfg])
  i_dn = np.array([rng.choice(np.flatnonzero(r < 0)) for r in cfg])
  u = rng.uniform(0, 1, b).astype(np.float32)
  mask = eng.mc_step_injected(i_up, i_dn, u)
  _, ref_mask, ratios = vo.mc_step(amp, cfg, i_up, i_dn, u)
  near = np.abs(ratios - np.sqrt(u.astype(np.float64))) < 1e-3 * np.maximum(ratios, 1e-30)
  np.testing.assert_array_equal(mask[~near], ref_mask[~near])
  cur, ok = cfg.copy(), np.ones(b, bool)
  for step in range(16):
    eng.set_configs(cur)
    pu, pd, pv = eng.debug_proposals(step)
    u_sites, u_acc = vo.step_uniforms(2024, np.arange(b), step, n)
    iu, idn = vo.propose_exchange(cur, u_sites)
    np.testing.assert_array_equal(pu, iu)
    np.testing.assert_array_equal(pd, idn)
    cur_next, _, ratios = vo.mc_step(amp, cur, iu, idn, u_acc)
    ok &= ~(np.abs(ratios - np.sqrt(u_acc.astype(np.float64))) < 1e-3 * np.maximum(ratios, 1e-30))
    cur = cur_next
  eng.set_configs(cfg)
  eng.step_counter = 0
  accepted = eng.mc_steps(16)
  got = eng.get_configs()
  assert ok.sum() > b // 2 and 0 < accepted < 16 * b
  np.testing.assert_array_equal(got[ok], cur[ok])
  eng.mc_steps(100)
  chains = eng.get_configs()
  assert (chains.sum(1) == 0).all()
  lc, pc = eng.amplitude()
  lr, pr = eng.amplitude(chains)
  np.testing.assert_array_equal(lc, lr)
  np.testing.assert_array_equal(pc, pr)
  eng.close()


def test_nnb_sampler_distribution_chi2_on_a_ring():
  """10-site ring: the sampled frequencies of the 252 Sz = 0 configurations against |psi|^2 (statistic and threshold of
  the pbdg test)."""
  n, l, h, b = 10, 1, 16, 2048
  theta = no.default_theta(n, l, h, 15)
  all_cfg = po.sz0_configurations(n)
  w = no.psi(theta, all_cfg, l, h) ** 2
  w /= w.sum()
  eng = _engine(n, b, l, h)
  eng.set_params(theta)
  eng.set_configs(vo.random_configurations(n, b, np.random.RandomState(16)))
  eng.mc_steps(200)
  index = {tuple(r.astype(int)): i for i, r in enumerate(all_cfg)}
  counts = np.zeros(len(all_cfg))
  for _ in range(10):
    eng.mc_steps(40)
    for r in eng.get_configs():
      counts[index[tuple(r.astype(int))]] += 1
  expect = w * counts.sum()
  keep = expect > 5
  chi2 = ((counts[keep] - expect[keep]) ** 2 / expect[keep]).sum()
  dof = keep.sum() - 1
  assert chi2 < 3.0 * (dof + 3.1 * np.sqrt(2 * dof)), (chi2, dof)
  eng.close()


def test_nnb_evaluate_matches_exact_energy_on_the_4x4_torus():
  n, l, h, b = 16, 1, 16, 1024
  bonds = vo.torus_bonds(4, 4)
  theta = no.default_theta(n, l, h, 17)
  exact = no.exact_energy(theta, bonds, 1.0, 1.0, n, l, h, po.sz0_configurations(n))
  eng = _engine(n, b, l, h)
  eng.set_params(theta); eng.set_bonds(bonds, 1.0, 1.0)
  eng.set_configs(vo.random_configurations(n, b, np.random.RandomState(18)))
  means, _ = eng.evaluate(None, 100, 20, 16)
  se = means.std(ddof=1) / np.sqrt(len(means))
  assert abs(means.mean() - exact) < 5 * se + 1e-6, (means.mean(), exact, se)
  eng.close()


def test_nnb_sharded_chains_match_one_ctx():
  n, l, h, b = 16, 2, 32, 64
  bonds = vo.torus_bonds(4, 4)
  theta = no.default_theta(n, l, h, 19)
  cfg = vo.random_configurations(n, b, np.random.RandomState(20))
  one = _engine(n, b, l, h)
  halves = [_engine(n, b // 2, l, h, chain_offset=r * (b // 2)) for r in range(2)]
  for r, eng in enumerate([one] + halves):
    eng.set_params(theta); eng.set_bonds(bonds, 1.0, 1.0)
    eng.set_configs(cfg if r == 0 else cfg[(r - 1) * (b // 2):r * (b // 2)])
    eng.mc_steps(20)
    eng.reset_accumulators()
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  np.testing.assert_array_equal(np.concatenate([x.get_configs() for x in halves]), one.get_configs())
  a = one.get_accumulators()
  s = halves[0].get_accumulators() + halves[1].get_accumulators()
  p = theta.size
  assert np.abs(s[:2 * p] - a[:2 * p]).max() <= 1e-5 * np.abs(a[:2 * p]).max() + 1e-6
  assert abs(s[2 * p] - a[2 * p]) <= 1e-5 * abs(a[2 * p]) + 1e-5 and s[2 * p + 1] == a[2 * p + 1]
  for eng in [one] + halves:
    eng.close()


def test_nnb_run_training_and_energy_evaluation(tmp_path, monkeypatch):
  """run_training --wavefunction_type=fully_connected_nnb on the 4 x 4 Heisenberg torus (jx = +1, exact E0 = -11.2285):
  EnergyGradient, then a short LogOverlapITSWO run; the evaluated energy is below the Neel state's -8.0; checkpoints
  reload from .npz and TF bundles; StochasticReconfiguration raises NotImplementedError."""
  from cgs_vmc_amd import lattice, run_energy_evaluation, run_training, session, wavefunctions
  monkeypatch.setenv('CGS_VMC_INIT_SEED', '7')
  hp = ('batch_size=512,num_equilibration_sweeps=10,num_batches_per_epoch=20,learning_rates=[0.003,0.001],'
        'learning_rate_stops=[80],num_evaluation_samples=20,num_fc_layers=2,fc_layer_size=32')
  for fmt, opt, epochs in (('npz', 'EnergyGradient', 120), ('tf', 'LogOverlapITSWO', 10)):
    monkeypatch.setenv('CGS_VMC_CHECKPOINT_FORMAT', fmt)
    session.reset_default_graph(); wavefunctions.reset_name_scope()
    d = str(tmp_path / fmt)
    os.makedirs(d)
    lattice.write_bonds(d, lattice.torus_bonds(4, 4))
    run_training.main(['--checkpoint_dir', d, '--num_sites', '16', '--heisenberg_jx', '1.0',
                       '--wavefunction_type', 'fully_connected_nnb', '--optimizer', opt,
                       '--num_epochs', str(epochs), '--hparams', hp])
    energies = [float(x) for x in open(os.path.join(d, 'metrics.txt')).read().split()]
    assert len(energies) == epochs and np.isfinite(energies).all()
    session.reset_default_graph(); wavefunctions.reset_name_scope()
    mean, _ = run_energy_evaluation.main(['--checkpoint_dir', d, '--heisenberg_jx', '1.0'])
    assert np.isfinite(mean)
    if fmt == 'npz':
      print('nnb 4x4 EnergyGradient: best epoch E %.4f, evaluated E %.4f' % (min(energies), mean))
      assert mean < -8.0, (mean, energies[-5:])
      assert mean > -11.2285 - 3 * 0.16, mean
    else:
      assert not any(f.endswith('.npz') for f in os.listdir(d))
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  d = str(tmp_path / 'sr')
  os.makedirs(d)
  lattice.write_bonds(d, lattice.torus_bonds(4, 4))
  with pytest.raises(NotImplementedError):
    run_training.main(['--checkpoint_dir', d, '--num_sites', '16', '--heisenberg_jx', '1.0',
                       '--wavefunction_type', 'fully_connected_nnb', '--optimizer', 'StochasticReconfiguration',
                       '--num_epochs', '2', '--hparams', 'batch_size=64,num_fc_layers=2,fc_layer_size=32'])


def test_nnb_refusals():
  from cgs_vmc_amd.engine import VmcEngine
  with pytest.raises(ValueError):
    _engine(15, 4, 2, 32)
  with pytest.raises(NotImplementedError):
    _engine(258, 4, 2, 32)
  with pytest.raises(NotImplementedError):
    _engine(16, 4, 0, 32)
  with pytest.raises(NotImplementedError):
    _engine(16, 4, 2, 1024)
  eng = _engine(16, 8, 2, 32)
  cfg = vo.random_configurations(16, 8, np.random.RandomState(21))
  bad = cfg.copy()
  bad[0, np.flatnonzero(bad[0] < 0)[0]] = 1.0
  eng.set_params(no.default_theta(16, 2, 32, 22))
  with pytest.raises(ValueError):
    eng.amplitude(bad)
  with pytest.raises(ValueError):
    eng.set_configs(bad)
  with pytest.raises(NotImplementedError):
    eng.sr_reserve(2)
  eng.close()
  # ansatz id 8 stays unassigned
  lib = _hip.load()
  import ctypes as C
  desc = _hip.VmcDesc(16, 8, 2, 32, 0, 1, 0, 0, 8, 0, 1, None, 0, 0, 0, 0)
  ctx = C.c_void_p()
  assert lib.vmc_create(C.byref(desc), C.byref(ctx)) == _hip.VMC_ERR_UNSUPPORTED

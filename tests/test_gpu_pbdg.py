"""GPU parity of the pbdg ansatz -- ProjectedBDG (wavefunctions.py:876-928) on csrc/pbdg.hip -- through the C ABI and
the training front end: amplitudes, local energies and accumulators against the fp64 oracle (tests/pbdg_oracle.py), the
sampler (injected steps, replayed chains, the cache it leaves, a chi^2 test of its distribution), exact <H> by
enumeration, sharded chains and run_training / run_energy_evaluation."""
import os

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import gnn_oracle as go
from tests import pbdg_oracle as po

pytestmark = pytest.mark.gpu

EPS32 = np.finfo(np.float32).eps


def _engine(n, b, **kw):
  from cgs_vmc_amd.engine import VmcEngine
  kw.setdefault('seed', 2024)
  return VmcEngine(n, b, 1, 1, ansatz='pbdg', **kw)


def _theta(n, seed):
  lim = np.sqrt(3.0 / n)
  return np.random.default_rng(seed).uniform(-lim, lim, n * n).astype(np.float32)


def _amplitudes_close(eng, theta, cfg):
  logit, psi = eng.amplitude(cfg)
  ref_l, ref_s = po.logit_sign(theta, cfg)
  kappa = po.condition_numbers(theta, cfg)
  n = cfg.shape[1] // 2
  bound = 64 * n * EPS32 * kappa
  err = np.abs(logit.astype(np.float64) - ref_l)
  assert (err <= bound).all(), (err.max(), bound[err.argmax()])
  sure = bound < 0.5
  assert sure.any()
  np.testing.assert_array_equal(np.sign(psi)[sure], ref_s[sure])
  np.testing.assert_allclose(np.abs(psi), np.exp(logit.astype(np.float64) + 10.0), rtol=1e-5, atol=1e-37)


@pytest.mark.parametrize('case', ['square-4x4', 'triangular-6x6', 'n256'])
def test_pbdg_amplitudes_match_the_fp64_oracle(case):
  n, b = {'square-4x4': (16, 64), 'triangular-6x6': (36, 48), 'n256': (256, 8)}[case]
  theta = _theta(n, 1)
  cfg = vo.random_configurations(n, b, np.random.RandomState(2))
  eng = _engine(n, b)
  assert eng.kernel_path() == 7 and eng.num_params == n * n
  eng.set_params(theta)
  eng.set_configs(cfg)
  _amplitudes_close(eng, theta, cfg)
  logit_c, psi_c = eng.amplitude()                       # the chains' cache: the same rows kernel
  logit_r, psi_r = eng.amplitude(cfg)
  np.testing.assert_array_equal(logit_c, logit_r)
  np.testing.assert_array_equal(psi_c, psi_r)
  eng.close()


def test_pbdg_singular_pairing_and_refusals():
  n = 12
  theta = _theta(n, 3).reshape(n, n)
  theta[1] = theta[0]                                    # two equal rows: singular wherever sites 0 and 1 are up
  cfg = vo.random_configurations(n, 40, np.random.RandomState(4))
  eng = _engine(n, 40)
  eng.set_params(theta.ravel())
  logit, psi = eng.amplitude(cfg)
  both = (cfg[:, 0] > 0) & (cfg[:, 1] > 0)
  assert both.any() and (psi[both] == 0).all() and np.isneginf(logit[both]).all()
  assert np.isfinite(psi).all() and np.isfinite(logit[~both]).all()
  bad = cfg.copy()
  bad[0, np.flatnonzero(bad[0] < 0)[0]] = 1.0
  with pytest.raises(ValueError):
    eng.amplitude(bad)
  with pytest.raises(ValueError):
    eng.set_configs(bad)
  with pytest.raises(NotImplementedError):
    eng.sr_reserve(2)
  eng.close()
  with pytest.raises(ValueError):
    _engine(15, 4)
  with pytest.raises(NotImplementedError):
    _engine(258, 4)


def _acc_close(got, acc, p):
  for g, r in ((got[:p], acc.g1_total), (got[p:2 * p], acc.g2_total)):
    tol = 2e-3 * np.abs(r).max() + 1e-4
    assert np.abs(g - r).max() < tol, (np.abs(g - r).max(), tol)


def test_pbdg_local_energies_and_accumulators():
  """Triangular 6 x 6 cluster with jx = +1 (frustrated: the signs matter), both optimizers' accumulators; ITSWO
  against a perturbed supervisor, so that some omega / psi ratios are negative."""
  n, b = 36, 64
  bonds = go.triangular_bonds(6, 6)
  theta = _theta(n, 5)
  cfg = vo.random_configurations(n, b, np.random.RandomState(6))
  eng = _engine(n, b)
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, 1.0, 1.0)
  eloc = eng.local_energy()[0]
  ref = po.local_energy(theta, cfg, bonds, 1.0, 1.0)
  np.testing.assert_allclose(eloc, ref, rtol=2e-3, atol=2e-3 * np.abs(ref).mean())
  acc = vo.Accumulators(theta.size, np.float64)
  po.energy_gradient_accumulate(acc, theta, cfg, bonds, 1.0, 1.0)
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  res = eng.get_accumulators()
  _acc_close(res, acc, theta.size)
  assert abs(res[2 * theta.size] - acc.e_total) < 2e-3 * max(1, abs(acc.e_total))
  eng.transfer_params()
  theta_w = (theta + 0.3 * np.random.default_rng(7).standard_normal(theta.size) * np.sqrt(3.0 / n)).astype(np.float32)
  eng.set_params(theta_w, _hip.VMC_OMEGA)
  eng.set_shift(-10.0, _hip.VMC_OMEGA)
  acc = vo.Accumulators(theta.size, np.float64)
  _, ratio = po.log_overlap_accumulate(acc, theta, theta_w, cfg, bonds, 1.0, 1.0, -10.0, -10.0, 0.05)
  assert (ratio < 0).any()
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.05)
  res = eng.get_accumulators()
  _acc_close(res, acc, theta.size)
  assert abs(res[2 * theta.size + 2] - acc.r_total) < 2e-3 * max(1, np.abs(ratio).sum())
  eng.close()


def test_pbdg_sampler_injected_replayed_and_cached():
  n, b = 16, 64
  theta = _theta(n, 8)
  amp = po.amp_fn(theta)
  cfg = vo.random_configurations(n, b, np.random.RandomState(9))
  eng = _engine(n, b)
  eng.set_params(theta); eng.set_configs(cfg)
  # 1. injected proposals: the oracle's accept masks except within rounding of the sqrt(u) threshold
  rng = np.random.default_rng(10)
  i_up = np.array([rng.choice(np.flatnonzero(r > 0)) for r in cfg])
  i_dn = np.array([rng.choice(np.flatnonzero(r < 0)) for r in cfg])
  u = rng.uniform(0, 1, b).astype(np.float32)
  mask = eng.mc_step_injected(i_up, i_dn, u)
  _, ref_mask, ratios = vo.mc_step(amp, cfg, i_up, i_dn, u)
  near = np.abs(ratios - np.sqrt(u.astype(np.float64))) < 1e-3 * np.maximum(ratios, 1e-30)
  np.testing.assert_array_equal(mask[~near], ref_mask[~near])
  # 3. replay from the debug proposals: identical chains except those that met a near-tie
  eng.set_configs(cfg)
  eng.step_counter = 0
  cur, ok = cfg.copy(), np.ones(b, bool)
  for step in range(24):
    eng.set_configs(cur)              # the proposal dump on the oracle's chains
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
  eng.mc_steps(24)
  got = eng.get_configs()
  assert ok.sum() > b // 2
  np.testing.assert_array_equal(got[ok], cur[ok])
  # 2. after 200 steps the cache equals vmc_amplitude on the returned chains bit for bit
  eng.mc_steps(200)
  chains = eng.get_configs()
  assert (chains.sum(1) == 0).all()
  lc, pc = eng.amplitude()
  lr, pr = eng.amplitude(chains)
  np.testing.assert_array_equal(lc, lr)
  np.testing.assert_array_equal(pc, pr)
  eng.close()


def test_pbdg_sampler_distribution_chi2_on_a_ring():
  """10-site ring: the sampled frequencies of the 252 Sz = 0 configurations against |psi|^2."""
  n, b = 10, 2048
  theta = _theta(n, 11)
  all_cfg = po.sz0_configurations(n)
  w = po.psi(theta, all_cfg, 0.0) ** 2
  w /= w.sum()
  eng = _engine(n, b)
  eng.set_params(theta)
  eng.set_configs(vo.random_configurations(n, b, np.random.RandomState(12)))
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
  # samples 40 steps apart are not independent: allow a generous factor over the 99.9 % quantile
  assert chi2 < 3.0 * (dof + 3.1 * np.sqrt(2 * dof)), (chi2, dof)
  eng.close()


def test_pbdg_evaluate_matches_exact_energy_on_the_4x4_torus():
  n, b = 16, 1024
  bonds = vo.torus_bonds(4, 4)
  theta = _theta(n, 13)
  exact = po.exact_energy(theta, bonds, 1.0, 1.0, n)
  eng = _engine(n, b)
  eng.set_params(theta); eng.set_bonds(bonds, 1.0, 1.0)
  eng.set_configs(vo.random_configurations(n, b, np.random.RandomState(14)))
  means, _ = eng.evaluate(None, 100, 20, 16)
  se = means.std(ddof=1) / np.sqrt(len(means))
  assert abs(means.mean() - exact) < 5 * se + 1e-6, (means.mean(), exact, se)
  eng.close()


def test_pbdg_sharded_chains_match_one_ctx():
  n, b = 16, 64
  bonds = vo.torus_bonds(4, 4)
  theta = _theta(n, 15)
  cfg = vo.random_configurations(n, b, np.random.RandomState(16))
  one = _engine(n, b)
  halves = [_engine(n, b // 2, chain_offset=r * (b // 2)) for r in range(2)]
  for r, eng in enumerate([one] + halves):
    eng.set_params(theta); eng.set_bonds(bonds, 1.0, 1.0)
    eng.set_configs(cfg if r == 0 else cfg[(r - 1) * (b // 2):r * (b // 2)])
    eng.mc_steps(20)
    eng.reset_accumulators()
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  np.testing.assert_array_equal(np.concatenate([h.get_configs() for h in halves]), one.get_configs())
  a = one.get_accumulators()
  s = halves[0].get_accumulators() + halves[1].get_accumulators()
  p = theta.size
  assert np.abs(s[:2 * p] - a[:2 * p]).max() <= 1e-5 * np.abs(a[:2 * p]).max() + 1e-6
  assert abs(s[2 * p] - a[2 * p]) <= 1e-5 * abs(a[2 * p]) + 1e-5 and s[2 * p + 1] == a[2 * p + 1]
  for eng in [one] + halves:
    eng.close()


def test_pbdg_run_training_and_energy_evaluation(tmp_path, monkeypatch):
  """run_training --wavefunction_type=pbdg, EnergyGradient, 4 x 4 Heisenberg torus (jx = +1, exact E0/N = -0.7018):
  E/N < -0.60 and never below the exact energy by more than 3 sigma; the checkpoints reload from .npz and TF
  bundles; StochasticReconfiguration raises NotImplementedError."""
  from cgs_vmc_amd import lattice, run_energy_evaluation, run_training, session, wavefunctions
  monkeypatch.setenv('CGS_VMC_INIT_SEED', '7')
  hp = ('batch_size=512,num_equilibration_sweeps=10,num_batches_per_epoch=20,learning_rates=[0.01,0.003],'
        'learning_rate_stops=[150],num_evaluation_samples=20')
  for fmt, epochs in (('npz', 250), ('tf', 20)):
    monkeypatch.setenv('CGS_VMC_CHECKPOINT_FORMAT', fmt)
    session.reset_default_graph(); wavefunctions.reset_name_scope()
    d = str(tmp_path / fmt)
    os.makedirs(d)
    lattice.write_bonds(d, lattice.torus_bonds(4, 4))
    run_training.main(['--checkpoint_dir', d, '--num_sites', '16', '--heisenberg_jx', '1.0',
                       '--wavefunction_type', 'pbdg', '--optimizer', 'EnergyGradient',
                       '--num_epochs', str(epochs), '--hparams', hp])
    energies = [float(x) for x in open(os.path.join(d, 'metrics.txt')).read().split()]
    assert len(energies) == epochs and np.isfinite(energies).all()
    session.reset_default_graph(); wavefunctions.reset_name_scope()
    mean, _ = run_energy_evaluation.main(['--checkpoint_dir', d, '--heisenberg_jx', '1.0'])
    if fmt == 'npz':
      print('pbdg 4x4 EnergyGradient: best epoch E/N %.4f, evaluated E/N %.4f' % (min(energies) / 16, mean / 16))
      assert mean / 16 < -0.60, (mean / 16, energies[-5:])
      assert mean / 16 > -0.7018 - 3 * 0.01, mean / 16
    else:
      assert not any(f.endswith('.npz') for f in os.listdir(d))
      assert abs(mean - energies[-1]) < 1.5, (mean, energies[-3:])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  d = str(tmp_path / 'sr')
  os.makedirs(d)
  lattice.write_bonds(d, lattice.torus_bonds(4, 4))
  with pytest.raises(NotImplementedError):
    run_training.main(['--checkpoint_dir', d, '--num_sites', '16', '--heisenberg_jx', '1.0',
                       '--wavefunction_type', 'pbdg', '--optimizer', 'StochasticReconfiguration',
                       '--num_epochs', '2', '--hparams', 'batch_size=64'])

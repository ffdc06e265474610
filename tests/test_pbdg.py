"""CPU: the pbdg ansatz's front end (ProjectedBDG, wavefunctions.py:876-928) -- registry, variable name and shape,
initialiser, odd-N refusal, checkpoint names -- and the fp64 oracle (tests/pbdg_oracle.py): sign convention,
exchange ratio and log-derivatives; its float32 emulations of the sampler and of the local energies, and the
conditions that tests/test_gpu_det_large.py presumes of its inputs (tests/det_large_cases.py)."""
import copy
import itertools
import os
import subprocess

import numpy as np
import pytest

from cgs_vmc_amd import session, tf_checkpoint, utils, wavefunctions
from oracle import vmc_oracle as vo
from tests import det_large_cases as dc
from tests import pbdg_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = np.finfo(np.float32).eps


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


# ----------------------------------------------------------------------------------------------------------------- #
# The float32 emulations behind tests/test_gpu_det_large.py, and that test's conditions on the oracle alone
# ----------------------------------------------------------------------------------------------------------------- #
def test_sampler_emulation_matches_direct_determinants_at_16_sites():
  """Every decision of the emulation at N = 16 (R = 16: several refreshes in 200 steps): both ratios against
  exchange_ratio_direct on the replayed chains, the decision rule, the bookkeeping of slots and the final chains."""
  n_sites, b, steps = 16, 6, 200
  theta = dc.theta(n_sites, 21)
  cfg = vo.random_configurations(n_sites, b, np.random.RandomState(22))
  em = po.sampler_emulation(theta, cfg, 77, steps)
  cur = cfg.copy()
  worst32 = worst64 = 0.0
  for s in range(steps):
    # the amplitude tests' float32 bound on ln|det M|, 64 n eps32 kappa(M), taken for the ratio of two of them
    bound = 64 * (n_sites // 2) * EPS32 * po.condition_numbers(theta, cur)
    u_sites, u_acc = vo.step_uniforms(77, np.arange(b), s, n_sites)
    i_up, i_dn = vo.propose_exchange(cur, u_sites)
    np.testing.assert_array_equal(em['i_up'][s], i_up)
    np.testing.assert_array_equal(em['i_dn'][s], i_dn)
    np.testing.assert_array_equal(em['u'][s], u_acc)
    for ch in range(b):
      ref = abs(po.exchange_ratio_direct(theta, cur[ch], i_up[ch], i_dn[ch]))
      worst64 = max(worst64, abs(em['rho64'][s, ch] - ref) / ref)
      worst32 = max(worst32, abs(float(em['rho32'][s, ch]) - ref) / (bound[ch] * max(1.0, ref)))
      if em['accept'][s, ch]:
        cur[ch, i_up[ch]], cur[ch, i_dn[ch]] = -1.0, 1.0
    np.testing.assert_array_equal(em['accept'][s], em['rho32'][s] > np.sqrt(em['u'][s]))
  np.testing.assert_array_equal(em['configs'], cur)
  assert em['accept'].sum(0).min() > 2 * po.refresh_interval(n_sites)       # every chain went through refreshes
  assert em['fresh'][0].all() and not em['fresh'].all()
  assert worst64 < 1e-9 and worst32 < 1.0, (worst64, worst32)


def test_fresh_inverse_float32_ratio_and_terms_match_the_oracle():
  """exchange_ratio_fp32 (sign included) against direct determinants, and diagonal + exchange_terms in fp64 against
  po.local_energy, which knows nothing of the parity factor: both parities of |a - b| occur."""
  n_sites = 16
  theta = dc.theta(n_sites, 23)
  cfg = vo.random_configurations(n_sites, 40, np.random.RandomState(24))
  rng = np.random.default_rng(25)
  parities = set()
  for row in cfg:
    a, b = int(rng.choice(np.flatnonzero(row > 0))), int(rng.choice(np.flatnonzero(row < 0)))
    ref = po.exchange_ratio_direct(theta, row, a, b)
    assert abs(float(po.exchange_ratio_fp32(theta, row, a, b)) - ref) < 1e-4 * max(1.0, abs(ref))
    parities.add((abs(a - b) - 1) & 1)
  assert parities == {0, 1}
  bonds = vo.torus_bonds(4, 4, next_nearest=True)
  jx = rng.uniform(-1, 1, len(bonds))
  jz = rng.uniform(-1, 1, len(bonds))
  e = po.diagonal_energy(cfg, bonds, jz) + po.exchange_terms(theta, cfg, bonds, jx).sum(1)
  np.testing.assert_allclose(e, po.local_energy(theta, cfg, bonds, jx, jz), rtol=1e-9, atol=1e-9)
  e32 = po.local_energy_fp32(theta, cfg, bonds, jx.astype(np.float32), jz.astype(np.float32))
  assert e32.dtype == np.float32
  np.testing.assert_allclose(e32, e, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize('n_sites', sorted(dc.SAMPLER))
def test_large_sampler_inputs_meet_the_caps_of_the_gpu_test(n_sites):
  """What tests/test_gpu_det_large.py presumes of its sampler inputs, on the emulation's own run: the stored band is
  the measured one, at most 3 % of the decisions lie inside delta, the acceptance rate is between 0.15 and 0.4, every
  chain has a decision with a site in a slot >= 64, and at N = 160 / 256 every chain accepts more than R + 10 moves
  (an in-launch refresh, then updates again)."""
  em = dc.emulation(n_sites)
  err = np.abs(em['rho32'].astype(np.float64) - em['rho64']).max()
  stored = dc.EMULATED_RATIO_ERROR[n_sites]
  # (the maximum moves with the BLAS's summation order; delta's factor 4 absorbs a factor 2 of it)
  assert stored / 2 <= err <= 2 * stored, (err, stored)
  inside = np.abs(em['rho64'] - np.sqrt(em['u'].astype(np.float64))) <= dc.delta(n_sites)
  rate = em['accept'].mean()
  fewest = em['accept'].sum(0).min()
  print('N = %d: max |rho32 - rho64| %.3g (stored %.3g), delta %.3g, %d of %d decisions inside, acceptance %.3f, '
        'fewest accepted moves %d' % (n_sites, err, stored, dc.delta(n_sites), inside.sum(), inside.size, rate, fewest))
  assert inside.mean() <= 0.03
  assert 0.15 <= rate <= 0.4
  assert ((em['slot_up'] >= 64) | (em['slot_dn'] >= 64)).any(0).all()
  if n_sites >= 160:
    assert fewest > po.refresh_interval(n_sites) + 10
    assert not em['fresh'][-1].any()                      # updating again after the refresh
  # the emulation's float32 decisions agree with the fp64 rule outside the band
  np.testing.assert_array_equal(em['accept'][~inside], (em['rho64'] > np.sqrt(em['u'].astype(np.float64)))[~inside])


@pytest.mark.parametrize('n_sites', sorted(dc.ELOC))
def test_large_local_energy_bound_is_measured_and_sharp(n_sites):
  """The stored c of the local-energy bound is the float32 emulation's, and the bound notices one wrong parity
  factor: flipping the sign of a single term moves E_loc by more than the bound -- for the median term of every row,
  and for at least 90 % of all terms."""
  theta, cfg, bonds, jx, jz = dc.eloc_inputs(n_sites)
  assert (jx == 0).sum() == 1 and (jx < 0).sum() == 1
  dist = np.array([abs(a - b) for a, b in bonds])
  assert set((dist - 1) & 1) == {0, 1} and dist.max() >= n_sites - 16
  terms = po.exchange_terms(theta, cfg, bonds, jx)
  diag = po.diagonal_energy(cfg, bonds, jz)
  e64 = diag + terms.sum(1)
  np.testing.assert_array_equal(diag, po.diagonal_energy(cfg, bonds, jz, np.float32))      # exact in float32
  e32 = po.local_energy_fp32(theta, cfg, bonds, jx, jz).astype(np.float64)
  ratio = (np.abs(e32 - e64) / (EPS32 * np.abs(terms).sum(1))).max()
  stored = dc.EMULATED_ELOC_RATIO[n_sites]
  assert stored / 2 <= ratio <= 2 * stored, (ratio, stored)
  bound = dc.eloc_bound(n_sites, terms, diag)
  assert (np.abs(e32 - e64) <= bound).all()
  shares = []
  for r in range(len(cfg)):
    live = np.flatnonzero(terms[r])
    mag = np.abs(terms[r, live])
    k = live[np.argsort(mag)[mag.size // 2]]
    flipped = diag[r] + po.exchange_terms(theta, cfg[r:r + 1], bonds, jx, flip=(0, k)).sum()
    assert abs(flipped - e64[r]) > bound[r], (r, k, flipped - e64[r], bound[r])
    shares.append((2 * mag > bound[r]).mean())
  print('N = %d: err / (eps32 sum|terms|) %.3g (stored %.3g); share of terms whose flip exceeds the bound: %s'
        % (n_sites, ratio, stored, np.round(shares, 3)))
  assert min(shares) >= 0.9

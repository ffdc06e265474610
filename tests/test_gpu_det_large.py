"""GPU: the determinant kernels above 64 pairs (n = N/2 > 64) -- csrc/pb_det.hpp, pbdg.hip, nnb.hip.  Above n = 64 every
column loop gains its second column group (the t = 1 half of pb_eliminate's and pb_update's register arrays), pb_lists
needs up to four ballots, a workgroup holds two chains (N = 130, 160) or one (N = 256), and at N = 256 a launch needs
the opt-in above 64 KiB of LDS.  The inputs and the measured bands are those of tests/det_large_cases.py; the
conditions on them (caps, sharpness) are proven on the CPU in tests/test_pbdg.py.

  sampler   every Metropolis decision of one T-step launch of k_pbdg_sweep, judged against the fp64 ratio of the same
            move within delta = 4 x the float32 emulation's largest ratio error (absolute, in units of the ratio);
  psi = 0   the sampler's branch for a chain at psi = 0 (factorise the candidate, revert on failure), N = 12 and 130;
  energies  k_pbdg_eloc within c eps32 sum|terms| per row, c = 8 x the fresh-inverse float32 emulation's worst, and the
            gradient sums (inv_out / pos_out into k_pbdg_grad_part) at N = 160 and 256;
  nnb       k_nnb_rows as amplitude, local-energy and write_delta rows at N = 130 and 160, and the bridge to pbdg at
            N = 160.

Measured on an MI355X: the figures are in the docstrings of the tests and in DESIGN.md ("Pinned by" of pbdg and nnb).
"""
import time

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import det_large_cases as dc
from tests import nnb_oracle as no
from tests import pbdg_oracle as po

pytestmark = pytest.mark.gpu

EPS32 = np.finfo(np.float32).eps


def _pbdg(n, b):
  from cgs_vmc_amd.engine import VmcEngine
  return VmcEngine(n, b, 1, 1, ansatz='pbdg', seed=dc.SEED)


def _nnb(n, b, l, h):
  from cgs_vmc_amd.engine import VmcEngine
  return VmcEngine(n, b, l, h, ansatz='fully_connected_nnb', seed=dc.SEED)


def _acc_close(got, acc, p, what):
  # the tolerance of tests/test_gpu_pbdg.py
  for name, g, r in (('g1', got[:p], acc.g1_total), ('g2', got[p:2 * p], acc.g2_total)):
    tol = 2e-3 * np.abs(r).max() + 1e-4
    err = np.abs(g - r).max()
    print('%s %s: max error %.3g, tolerance %.3g, error / tolerance %.3g' % (what, name, err, tol, err / tol))
    assert err < tol, (what, name, err, tol)


# ------------------------------------------------------------------------------------------------ sampler decisions
@pytest.mark.parametrize('n_sites', sorted(dc.SAMPLER))
def test_pbdg_sampler_decisions_above_64_pairs(n_sites):
  """Launches of k = 1 .. T steps from the same chains and step counter 0: a launch factorises only at its start, so
  the k-th step of every longer launch is made with M^-1 as k - 1 in-launch rank-2 updates (and the refreshes every R
  accepted moves) left it, and X_k - X_{k-1} is the T-step launch's k-th decision.  Asserted: each X_k differs from
  X_{k-1} per chain by nothing or by exactly the exchange the oracle proposes from X_{k-1}; the decisions sum to the
  accepted count of the T-step launch; every decision equals rho > sqrt(u) for the fp64 rho = |psi'/psi| of its own
  move wherever |rho - sqrt(u)| > delta; at most 3 % of the decisions lie inside delta.

  Measured on an MI355X (N: delta, decisions inside it, decisions against the fp64 rule at any distance, the smallest
  band that would have passed, time of the T launches): 130: 1.17e-3, 1 of 600, 0, 0, 0.24 s; 160: 4.36e-3, 11 of 2400,
  0, 0, 2.5 s; 256: 1.45e-2, 24 of 2304, 0, 0, 5.7 s (T = 640 took 6.8 s and was shortened to 576, the fewest accepted
  moves of a chain 144 > R + 10 = 138).  Acceptance 0.300 / 0.263 / 0.268."""
  theta, cfg0, steps = dc.sampler_inputs(n_sites)
  b = len(cfg0)
  eng = _pbdg(n_sites, b)
  eng.set_params(theta)
  t0 = time.perf_counter()
  xs, accepted = [cfg0], 0
  for k in range(1, steps + 1):
    eng.set_configs(cfg0)
    eng.step_counter = 0
    accepted = eng.mc_steps(k)
    xs.append(eng.get_configs())
  gpu_seconds = time.perf_counter() - t0
  rows = np.arange(b)
  decided = np.zeros((steps, b), bool)
  rho = np.zeros((steps, b))
  root_u = np.zeros((steps, b))
  logit = po.logit_sign(theta, cfg0)[0]
  for k in range(1, steps + 1):
    prev, cur = xs[k - 1], xs[k]
    u_sites, u_acc = vo.step_uniforms(dc.SEED, rows, k - 1, n_sites)
    i_up, i_dn = vo.propose_exchange(prev, u_sites)
    cand = prev.copy()
    cand[rows, i_up], cand[rows, i_dn] = -1.0, 1.0
    moved = (cur != prev).any(1)
    np.testing.assert_array_equal(cur[moved], cand[moved])          # nothing, or exactly the proposed exchange
    logit_cand = po.logit_sign(theta, cand)[0]
    decided[k - 1], rho[k - 1], root_u[k - 1] = moved, np.exp(logit_cand - logit), np.sqrt(u_acc.astype(np.float64))
    logit = np.where(moved, logit_cand, logit)
  assert decided.sum() == accepted, (decided.sum(), accepted)
  delta = dc.delta(n_sites)
  gap = np.abs(rho - root_u)
  inside = gap <= delta
  wrong = decided != (rho > root_u)
  band = gap[wrong].max() if wrong.any() else 0.0
  print('N = %d, T = %d, %d chains: %.2f s for the %d launches; acceptance %.3f, fewest accepted moves of a chain %d; '
        'delta %.3g, %d of %d decisions inside it (cap 3 %%), %d decisions against the fp64 rule, the smallest band '
        'that passes %.3g' % (n_sites, steps, b, gpu_seconds, steps, decided.mean(), decided.sum(0).min(), delta,
                              inside.sum(), inside.size, wrong.sum(), band))
  assert inside.mean() <= 0.03, (inside.sum(), inside.size)
  assert 0.15 <= decided.mean() <= 0.4
  if n_sites >= 160:
    assert decided.sum(0).min() > po.refresh_interval(n_sites) + 10  # through an in-launch refresh and beyond
  bad = wrong & ~inside
  if bad.any():
    # drift or inherent float32 error?  the same states judged by one-step launches (a fresh inverse)
    fresh_wrong = 0
    for k, ch in zip(*np.nonzero(bad)):
      eng.set_configs(xs[k])
      eng.step_counter = int(k)
      eng.mc_steps(1)
      fresh_wrong += int((eng.get_configs()[ch] != xs[k][ch]).any() != (rho[k, ch] > root_u[k, ch]))
    raise AssertionError('%d decisions outside delta = %.3g disagree with the fp64 rule (the smallest band that passes: '
                         '%.3g); %d of them also from a fresh inverse' % (bad.sum(), delta, band, fresh_wrong))
  eng.close()


# ------------------------------------------------------------------------------------------------ the psi = 0 branch
@pytest.mark.parametrize('n_sites,b', [(12, 6), (130, 5)])
def test_pbdg_sampler_at_zero_amplitude(n_sites, b):
  """Rows 0 and 1 of F equal and both sites up: psi = 0.  A proposal that lowers one of the two leads to psi' != 0 and
  is accepted whatever u is (|psi'| / 0 = inf), one that leaves both up has psi' = 0 and is rejected (0 / 0 = NaN) with
  the chain unchanged -- vo.mc_step's semantics.  Then 50 free steps: Sz = 0, no NaN, and the cache equals
  vmc_amplitude on the returned chains bit for bit."""
  f = dc.theta(n_sites, 31).reshape(n_sites, n_sites)
  f[1] = f[0]
  theta = f.ravel()
  rng = np.random.default_rng(32)
  chains = -np.ones((b, n_sites), np.float32)
  chains[:, :2] = 1.0
  for row in chains:
    row[2 + rng.choice(n_sites - 2, n_sites // 2 - 2, replace=False)] = 1.0

  def amp(c):      # det M = 0 exactly wherever two rows of M are equal
    return np.where((c[:, 0] > 0) & (c[:, 1] > 0), 0.0, po.psi(theta, c))

  eng = _pbdg(n_sites, b)
  eng.set_params(theta)
  eng.set_configs(chains)
  logit, psi = eng.amplitude()
  assert (psi == 0).all() and np.isneginf(logit).all()
  i_dn = np.array([rng.choice(np.flatnonzero(r < 0)) for r in chains])
  u = rng.uniform(0, 1, b).astype(np.float32)
  u[0], u[1] = np.float32(1.0) - np.float32(2.0 ** -24), 0.0      # the largest uniform of the generator, and zero
  # 1. lower site 0 or site 1: the candidate is nonsingular
  i_up = np.arange(b) % 2
  mask = eng.mc_step_injected(i_up, i_dn, u)
  want, ref_mask, ratios = vo.mc_step(amp, chains, i_up, i_dn, u)
  assert np.isinf(ratios).all() and ref_mask.all()
  np.testing.assert_array_equal(mask, ref_mask)
  np.testing.assert_array_equal(eng.get_configs(), want)
  logit, psi = eng.amplitude()
  assert np.isfinite(logit).all() and (psi != 0).all()
  # 2. lower another up site: both stay up, the candidate is singular too
  eng.set_configs(chains)
  i_up = np.array([rng.choice(np.flatnonzero(r[2:] > 0)) + 2 for r in chains])
  mask = eng.mc_step_injected(i_up, i_dn, u)
  want, ref_mask, ratios = vo.mc_step(amp, chains, i_up, i_dn, u)
  assert np.isnan(ratios).all() and not ref_mask.any()
  np.testing.assert_array_equal(mask, ref_mask)
  np.testing.assert_array_equal(eng.get_configs(), chains)
  # 3. free steps from psi = 0
  eng.set_configs(chains)
  eng.step_counter = 0
  eng.mc_steps(50)
  got = eng.get_configs()
  assert (got.sum(1) == 0).all() and (np.abs(got) == 1).all()
  left = ~((got[:, 0] > 0) & (got[:, 1] > 0))
  print('N = %d: %d of %d chains left psi = 0 within 50 steps' % (n_sites, left.sum(), b))
  lc, pc = eng.amplitude()
  lr, pr = eng.amplitude(got)
  assert not np.isnan(lc).any() and not np.isnan(pc).any()
  np.testing.assert_array_equal(lc, lr)
  np.testing.assert_array_equal(pc, pr)
  assert ((pc != 0) == left).all()
  eng.close()


# ------------------------------------------------------------------------------------- local energies, gradient sums
@pytest.mark.parametrize('n_sites', sorted(dc.ELOC))
def test_pbdg_local_energies_and_gradient_sums_above_64_pairs(n_sites):
  """16 x 10 and 16 x 16 torus with nearest and next-nearest bonds and per-bond couplings: E_loc of every row within
  c eps32 sum_q |term_q| + one rounding of the sum (tests/det_large_cases.eloc_bound; tests/test_pbdg.py shows that one
  term with the wrong parity factor exceeds it), against the fp64 oracle's slogdet route, which has no parity factor;
  the energy-gradient accumulators (M^-1 and the slots through inv_out / pos_out) under the suite's tolerance.

  Measured on an MI355X, worst row: error / bound 0.031 (N = 160) and 0.079 (N = 256); error / (eps32 sum|terms|) 8.0
  and 67 (kappa 3.0e3 and 3.8e3) against c = 257 and 848: the float32 error of the elimination (eliminate_fp32 shows
  32 and 106 on the same rows).  Gradient sums: error / tolerance at most 0.009 and 0.051.  Each case under half a
  second."""
  theta, cfg, bonds, jx, jz = dc.eloc_inputs(n_sites)
  acc = vo.Accumulators(theta.size, np.float64)
  ref = po.energy_gradient_accumulate(acc, theta, cfg, bonds, jx, jz)
  terms = po.exchange_terms(theta, cfg, bonds, jx)
  diag = po.diagonal_energy(cfg, bonds, jz)
  assert np.abs(diag + terms.sum(1) - ref).max() < 1e-9 * np.abs(terms).sum(1).max()
  bound = dc.eloc_bound(n_sites, terms, diag)
  eng = _pbdg(n_sites, len(cfg))
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, jx, jz)
  t0 = time.perf_counter()
  eloc = eng.local_energy()[0]
  seconds = time.perf_counter() - t0
  err = np.abs(eloc.astype(np.float64) - ref)
  print('N = %d: E_loc error / bound per row %s (error / (eps32 sum|terms|) %s, kappa %s), %.3f s'
        % (n_sites, np.round(err / bound, 3), np.round(err / (EPS32 * np.abs(terms).sum(1)), 2),
           np.round(po.condition_numbers(theta, cfg)), seconds))
  assert (err <= bound).all(), (err, bound)
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  res = eng.get_accumulators()
  _acc_close(res, acc, theta.size, 'pbdg N = %d' % n_sites)
  e_err, e_tol = abs(res[2 * theta.size] - acc.e_total), 2e-3 * max(1, abs(acc.e_total))
  print('pbdg N = %d e_total: error %.3g, tolerance %.3g' % (n_sites, e_err, e_tol))
  assert e_err < e_tol
  eng.close()


# ---------------------------------------------------------------------------------------------------------------- nnb
@pytest.mark.parametrize('n_sites', sorted(dc.NNB_TORUS))
def test_nnb_rows_above_64_pairs(n_sites):
  """L = 2, H = 16 at N = 130 and 160, five rows (an idle wave in the last workgroup), a backflow of a few per cent on a
  uniform pairing matrix (det_large_cases.nnb_inputs): amplitudes as in test_nnb_amplitudes_match_the_fp64_oracle (signs
  equal, 64 n eps32 kappa on every row); local energies (k_nnb_rows with val) within c eps32 sum|terms| + one rounding
  of the sum, c = 8 x the worst of the float32 emulation of these rows (nnb_oracle.exchange_terms; tests/test_nnb.py
  shows that one term of the wrong sign exceeds it); energy-gradient accumulators (write_delta) under the suite's
  tolerance.

  Measured on an MI355X, worst row: |dlogit| 0.0044 and 0.0021 n eps32 kappa; E_loc error / bound 0.080 and 0.193
  (error / (eps32 sum|terms|) 14.6 and 25.9 against c = 182 and 134); gradient sums error / tolerance 0.010 and
  0.006."""
  l, h = dc.NNB_LAYERS, dc.NNB_UNITS
  theta, cfg, bonds, jx, jz = dc.nnb_inputs(n_sites)
  eng = _nnb(n_sites, len(cfg), l, h)
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, jx, jz)
  logit, psi = eng.amplitude(cfg)
  ref_l, ref_s = no.logit_sign(theta, cfg, l, h)
  kappa = no.condition_numbers(theta, cfg, l, h)
  err = np.abs(logit.astype(np.float64) - ref_l)
  print('nnb N = %d: max of |dlogit| / (n eps32 kappa) %.3g (bound 64), max kappa %.3g'
        % (n_sites, (err / ((n_sites // 2) * EPS32 * kappa)).max(), kappa.max()))
  assert (err <= 64 * (n_sites // 2) * EPS32 * kappa).all()
  np.testing.assert_array_equal(np.where(np.signbit(psi), -1.0, 1.0), ref_s)
  logit_c, psi_c = eng.amplitude()
  np.testing.assert_array_equal(logit_c, logit)
  np.testing.assert_array_equal(psi_c, psi)
  acc = vo.Accumulators(theta.size, np.float64)
  ref = no.energy_gradient_accumulate(acc, theta, cfg, bonds, jx, jz, l, h)
  terms = no.exchange_terms(theta, cfg, bonds, jx, l, h)
  diag = po.diagonal_energy(cfg, bonds, jz)
  assert np.abs(diag + terms.sum(1) - ref).max() < 1e-9 * np.abs(terms).sum(1).max()
  bound = dc.nnb_eloc_bound(n_sites, terms, diag)
  eloc = eng.local_energy()[0]
  e_err = np.abs(eloc.astype(np.float64) - ref)
  print('nnb N = %d: E_loc error / bound per row %s, error / (eps32 sum|terms|) %s'
        % (n_sites, np.round(e_err / bound, 3), np.round(e_err / (EPS32 * np.abs(terms).sum(1)), 1)))
  assert (e_err <= bound).all(), (e_err, bound)
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  res = eng.get_accumulators()
  _acc_close(res, acc, theta.size, 'nnb N = %d' % n_sites)
  assert abs(res[2 * theta.size] - acc.e_total) < 2e-3 * max(1, abs(acc.e_total))
  eng.close()


def test_nnb_bridge_to_pbdg_at_160_sites():
  """W_out = 0, b_out = F on the inputs of the N = 160 local-energy test: the nnb ctx forms every term from two fresh
  determinants (k_nnb_rows, two column groups), the pbdg ctx from the 2 x 2 determinant with the parity factor
  (k_pbdg_eloc).  Amplitudes: signs equal and the logits within 64 n eps32 kappa of each other; both ctxs' local energies
  within the bound of the local-energy test of the fp64 oracle; the b_out block of nnb's gradient sums against pbdg's
  under the suite's tolerance.  Measured on an MI355X: identical logits, E_loc error / bound at most 0.015 (nnb) and
  0.031 (pbdg), the b_out block within 0.5 % of the tolerance."""
  n, l, h = 160, dc.NNB_LAYERS, dc.NNB_UNITS
  f, cfg, bonds, jx, jz = dc.eloc_inputs(n)
  b = len(cfg)
  theta = no.default_theta(n, l, h, 4)
  ow, ob = no.offsets(n, l, h)
  theta[ow:ob] = 0.0
  theta[ob:] = f
  eng, ref = _nnb(n, b, l, h), _pbdg(n, b)
  ref.set_shift(0.0)
  for e, t in ((eng, theta), (ref, f)):
    e.set_params(t); e.set_configs(cfg); e.set_bonds(bonds, jx, jz)
  (lg, ps), (lr, pr) = eng.amplitude(), ref.amplitude()
  kappa = po.condition_numbers(f, cfg)
  d = np.abs(lg.astype(np.float64) - lr)
  print('bridge N = 160: max |logit_nnb - logit_pbdg| / (n eps32 kappa) %.3g' % (d / ((n // 2) * EPS32 * kappa)).max())
  assert (d <= 64 * (n // 2) * EPS32 * kappa).all()
  np.testing.assert_array_equal(np.sign(ps), np.sign(pr))
  np.testing.assert_array_equal(np.sign(pr), po.logit_sign(f, cfg)[1])
  terms = po.exchange_terms(f, cfg, bonds, jx)
  diag = po.diagonal_energy(cfg, bonds, jz)
  bound = dc.eloc_bound(n, terms, diag)
  exact = diag + terms.sum(1)
  for name, e in (('nnb', eng), ('pbdg', ref)):
    err = np.abs(e.local_energy()[0].astype(np.float64) - exact)
    print('bridge N = 160, %s: E_loc error / bound per row %s' % (name, np.round(err / bound, 3)))
    assert (err <= bound).all(), (name, err, bound)
  for e in (eng, ref):
    e.reset_accumulators()
    e.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  a, r = eng.get_accumulators(), ref.get_accumulators()
  p = theta.size
  for name, got, want in (('g1', a[ob:p], r[:n * n]), ('g2', a[p + ob:2 * p], r[n * n:2 * n * n])):
    err, tol = np.abs(got - want).max(), 2e-3 * np.abs(want).max() + 1e-4
    print('bridge N = 160 %s (b_out block): max error %.3g, tolerance %.3g' % (name, err, tol))
    assert err < tol
  eng.close(); ref.close()

"""fp64 restatement in numpy of the overlap estimator (vmc_overlap, mode PENALIZED_ENERGY of vmc_accumulate), independent of
csrc/overlap.hip.  Helper of tests/test_overlap.py and tests/test_gpu_state_overlap.py; no tests of its own.

With r_c = phi(x_c) / psi(x_c) over chains x_c drawn from |psi|^2:
  F = |<phi|psi>|^2 / (<psi|psi><phi|phi>) = <r>^2 / <r^2> ~ S1^2 / (alive S2),  S1 = sum_c r_c,  S2 = sum_c r_c^2
  d(E + lam F) = 2 Cov(w, O),  w_c = E_loc(c) + lam (S1 / S2) r_c,  O = d ln psi / d theta
Every function takes an optional `weight` [B] (default 1 per chain): the exact weights psi^2 / sum psi^2 of an enumerated
basis turn the sums into the exact expectation values."""
import collections

import numpy as np

Ratios = collections.namedtuple('Ratios', ['d', 's', 'alive'])
"""d [B] fp64 = ln|r_c| (0 where s = 0), s [B] int = the sign of r_c (0: phi vanishes, or the chain is dead), alive [B]
bool = the chain's own amplitude does not vanish."""


def ratios(logit_psi, sign_psi, shift_psi, logit_om, sign_om, shift_om) -> Ratios:
  """From the two amplitude caches as the engine reports them: fp32 logits ln|psi| + shift, signs (or amplitudes: only their
  sign is read; None: an unsigned type) and the fp32 exponent shifts.  d = (logit_om - shift_om) - (logit_psi - shift_psi),
  each fp32 input widened to fp64 first."""
  lp, lo = np.asarray(logit_psi, np.float32).astype(np.float64), np.asarray(logit_om, np.float32).astype(np.float64)
  sp = np.ones(lp.shape, np.int64) if sign_psi is None else np.sign(np.asarray(sign_psi, np.float64)).astype(np.int64)
  so = np.ones(lp.shape, np.int64) if sign_om is None else np.sign(np.asarray(sign_om, np.float64)).astype(np.int64)
  s = sp * so
  with np.errstate(invalid='ignore'):
    d = (lo - np.float64(np.float32(shift_om))) - (lp - np.float64(np.float32(shift_psi)))
  return Ratios(np.where(s != 0, d, 0.0), s, sp != 0)


def sums(r: Ratios, weight=None):
  """{'s1', 's2', 'alive', 'log_scale', 'ratio'}: log_scale = max d over the chains with a ratio (0 when there is none),
  ratio [B] = s exp(d - log_scale), s1 = sum ratio, s2 = sum ratio^2, alive = the (weighted) number of chains alive."""
  w = np.ones(len(r.d)) if weight is None else np.asarray(weight, np.float64)
  has = r.s != 0
  m = float(r.d[has].max()) if has.any() else 0.0
  ratio = np.where(has, r.s * np.exp(np.where(has, r.d - m, 0.0)), 0.0)
  return {'s1': float((w * ratio).sum()), 's2': float((w * ratio * ratio).sum()), 'alive': float((w * r.alive).sum()),
          'log_scale': m, 'ratio': ratio}


def fidelity(r: Ratios, weight=None) -> float:
  v = sums(r, weight)
  return v['s1'] ** 2 / (v['alive'] * v['s2']) if v['s2'] > 0 and v['alive'] > 0 else 0.0


def weights(eloc, r: Ratios, lam, weight=None, dtype=np.float32):
  """w [B] = E_loc + lam (S1 / S2) ratio in fp64, rounded once to `dtype`; a dead chain, and every chain when S2 = 0,
  keeps E_loc."""
  v = sums(r, weight)
  w = np.asarray(eloc, np.float64).copy()
  if v['s2'] > 0:
    w = w + np.where(r.alive, float(lam) * (v['s1'] / v['s2']) * v['ratio'], 0.0)
  return w.astype(dtype)


def penalized_gradient(g1, g2, w_total, counts):
  """mean(g2) - mean(w) mean(g1) from the accumulators: g1 = sum_b O, g2 = sum_b w O over `counts` = (w_count, g_count) --
  the chains behind w_total and the accumulate calls behind g1 / g2 (the batch-sum convention of the energy gradient, no
  factor 2)."""
  w_count, g_count = counts
  g1, g2 = np.asarray(g1, np.float64), np.asarray(g2, np.float64)
  return g2 / g_count - (float(w_total) / float(w_count)) * g1 / g_count

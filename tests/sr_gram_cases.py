"""fp64 references of the sample-space stochastic reconfiguration (cgs_vmc_amd/csrc/srgram.hip), shared by
tests/test_sr_gram.py (CPU), tests/test_gpu_sr_gram.py and tests/test_gpu_sr_gram_shapes.py.

With n samples, centred log-derivatives Obar = O - 1 obar^T and eps = E - mean(E),

  x = (Obar^T Obar / n + lambda I)^-1 Obar^T eps / n  =  Obar^T (Obar Obar^T + n lambda I)^-1 eps

and the uncentred Gram matrix T = O O^T comes from the per-layer activations a_l and back-propagated deltas alone:

  T[b][b'] = sum_l (a_{l-1}[b] . a_{l-1}[b'] + 1) (delta_l[b] . delta_l[b'])  +  (a_last[b] . a_last[b'] + 1)

(a_last: the last activations for fully_connected -- the w_out, b_out block -- and the configuration for rbm -- the
w_on, b_on block).
"""
import numpy as np

from oracle import vmc_oracle as vo


def layer_terms(theta, cfgs, h, L, ansatz='fully_connected', nonlinearity='relu', dtype=np.float64):
  """([(a_{l-1}, delta_l) for every layer, first to last], a_last) in `dtype`: what the dense sample store holds."""
  x = np.asarray(cfgs, dtype)
  th = np.asarray(theta, dtype)
  dact = vo._NONLIN_DERIV[nonlinearity]
  terms = []
  if ansatz == 'rbm':
    hidden = vo.rbm_unpack(th, x.shape[1], h, L)[1:]
    _, zs, acts, z_last = vo.rbm_logit(th, x, h, L, nonlinearity, dtype, True)
    delta = np.tanh(z_last)
    for l in range(L, -1, -1):
      terms.insert(0, (acts[l], delta.copy()))
      if l > 0:
        delta = (delta @ hidden[l][0].T) * dact(zs[l - 1], acts[l])
    return terms, x
  assert ansatz == 'fully_connected'
  layers = vo.unpack(th, x.shape[1], h, L)
  _, zs, acts = vo.fc_logit(th, x, h, L, nonlinearity, dtype, True)
  delta = np.broadcast_to(layers[-1][0][:, 0][None, :], acts[-1].shape).copy()
  for l in range(L - 1, -1, -1):
    delta = delta * dact(zs[l], acts[l + 1])
    terms.insert(0, (acts[l], delta.copy()))
    if l > 0:
      delta = delta @ layers[l][0].T
  return terms, acts[-1]


def gram_ref(theta, cfgs, h, L, ansatz='fully_connected', nonlinearity='relu'):
  """T = O O^T [n][n] in fp64 by the per-layer formula, O never formed."""
  terms, a_last = layer_terms(theta, cfgs, h, L, ansatz, nonlinearity)
  t = a_last @ a_last.T + 1.0
  for a, d in terms:
    t = t + (a @ a.T + 1.0) * (d @ d.T)
  return t


def gram_magnitude(theta, cfgs, h, L, ansatz='fully_connected', nonlinearity='relu'):
  """M = |a_last| |a_last|^T + 1 + sum_l (|a| |a|^T + 1) o (|delta| |delta|^T) in fp64: the sum of the absolute products
  behind each entry of T, the scale a rounding error of that entry is measured on (M >= |T| elementwise)."""
  terms, a_last = layer_terms(theta, cfgs, h, L, ansatz, nonlinearity)
  a_last = np.abs(a_last)
  m = a_last @ a_last.T + 1.0
  for a, d in terms:
    a, d = np.abs(a), np.abs(d)
    m = m + (a @ a.T + 1.0) * (d @ d.T)
  return m


def gram_fp32(theta, cfgs, h, L, ansatz='fully_connected', nonlinearity='relu'):
  """gram_ref's formula in numpy float32 from end to end (forward pass, deltas, products): what plain fp32 arithmetic
  makes of T, the measured baseline of the per-element bound of tests/test_gpu_sr_gram_shapes.py."""
  terms, a_last = layer_terms(theta, cfgs, h, L, ansatz, nonlinearity, np.float32)
  one = np.float32(1.0)
  t = a_last @ a_last.T + one
  for a, d in terms:
    assert a.dtype == np.float32 and d.dtype == np.float32
    t = t + (a @ a.T + one) * (d @ d.T)
  assert t.dtype == np.float32
  return t


def per_sample_grads(theta, cfgs, h, L, ansatz='fully_connected', nonlinearity='relu'):
  fn = vo.rbm_per_sample_logit_grads if ansatz == 'rbm' else vo.per_sample_logit_grads
  return fn(theta, cfgs, h, L, nonlinearity=nonlinearity)


def per_sample_grads_from_terms(theta, cfgs, h, L, ansatz='fully_connected', nonlinearity='relu'):
  """O [n][P] of per_sample_grads assembled from layer_terms in the theta layout (per layer a (x) delta, then delta; the
  output block [a_last, 1] last for fully_connected, the onsite block [x, 1] first for rbm): the same numbers without
  rbm_per_sample_logit_grads' pass per row, for the cases of a thousand rows."""
  terms, a_last = layer_terms(theta, cfgs, h, L, ansatz, nonlinearity)
  n = a_last.shape[0]
  pieces = []
  for a, d in terms:
    pieces += [(a[:, :, None] * d[:, None, :]).reshape(n, -1), d]
  last = [a_last, np.ones((n, 1))]
  return np.concatenate(last + pieces if ansatz == 'rbm' else pieces + last, axis=1)


def _centre(m):
  return m - m.mean(0, keepdims=True)


def solve_samples_ref(o, e, lam):
  """x by the direct fp64 solve of the n x n system."""
  o = np.asarray(o, np.float64)
  e = np.asarray(e, np.float64)
  n = o.shape[0]
  oc = _centre(o)
  y = np.linalg.solve(oc @ oc.T + n * lam * np.eye(n), e - e.mean())
  return oc.T @ y


def centred_operator(t, lam):
  """C T C + n lambda I as a dense fp64 matrix."""
  t = np.asarray(t, np.float64)
  n = t.shape[0]
  c = np.eye(n) - np.full((n, n), 1.0 / n)
  return c @ t @ c + n * lam * np.eye(n)


def cg_samples_ref(t, e, lam, tol, max_iter, history=False):
  """The recurrence of the HIP path in fp64 on C T C + n lambda I (y0 = 0, stop at |r| <= tol |eps|).
  Returns (t_weights = y - mean(y), iterations): x = O^T t_weights.  With history=True a third value: the list, for
  k = 0 .. iterations, of (y_k - mean(y_k), sqrt(rr_k / rr_0)) -- what a solve cut short at max_iter = k returns."""
  a = centred_operator(t, lam)
  e = np.asarray(e, np.float64)
  eps = e - e.mean()
  y = np.zeros_like(eps); r = eps.copy(); p = eps.copy()
  rr0 = rr = r @ r
  it = 0
  hist = [(y - y.mean(), 1.0 if rr0 > 0 else 0.0)]
  while it < max_iter and rr > tol * tol * rr0 and rr0 > 0:
    q = a @ p
    alpha = rr / (p @ q)
    y += alpha * p
    r -= alpha * q
    rr_new = r @ r
    p = r + (rr_new / rr) * p
    rr = rr_new
    it += 1
    if history:
      hist.append((y - y.mean(), float(np.sqrt(rr / rr0))))
  if history:
    return y - y.mean(), it, hist
  return y - y.mean(), it


KINK = 1e-4      # draw_rows: a relu row is redrawn when a hidden pre-activation lies this close to 0


def min_preactivation(theta, cfgs, h, L, ansatz='fully_connected', nonlinearity='relu'):
  """Per row, the smallest fp64 |z| over all hidden units in front of the hidden activation (inf without such a unit)."""
  x = np.asarray(cfgs, np.float64)
  th = np.asarray(theta, np.float64)
  zs = (vo.rbm_logit if ansatz == 'rbm' else vo.fc_logit)(th, x, h, L, nonlinearity, np.float64, True)[1]
  out = np.full(x.shape[0], np.inf)
  for z in zs:
    out = np.minimum(out, np.abs(z).min(1))
  return out


def draw_rows(ansatz, theta, n_sites, h, L, rows, seed, nonlinearity='relu'):
  """(`rows` configurations, number of rejected draws) from the vo.random_configurations stream of RandomState(seed).
  For relu a row whose smallest fp64 hidden pre-activation |z| is below KINK is drawn again from the same stream: an fp32
  forward may land on the other side of the kink there, and a flipped derivative is not a rounding error.  This chooses
  inputs (tests/test_sr_gram.py bounds the rejected share); the smooth activations take every row."""
  rng = np.random.RandomState(seed)
  cfgs = vo.random_configurations(n_sites, rows, rng)
  rejected = 0
  while nonlinearity == 'relu':
    bad = np.nonzero(min_preactivation(theta, cfgs, h, L, ansatz, nonlinearity) < KINK)[0]
    if bad.size == 0:
      break
    rejected += bad.size
    cfgs[bad] = vo.random_configurations(n_sites, bad.size, rng)
  return cfgs, rejected


def make_theta(ansatz, n, h, L, seed=0, noise=0.05):
  """init + a `noise` perturbation, as make_case and tests/test_gpu_sr_gram.py::_case make it."""
  rng = np.random.default_rng(seed)
  theta = (vo.rbm_init_params if ansatz == 'rbm' else vo.init_params)(n, h, L, rng)
  return theta + (noise * rng.standard_normal(theta.size)).astype(np.float32)


def make_case(ansatz, n, h, L, rows, seed=0, noise=0.05):
  """Parameters as tests/test_gpu_sr.py::_setup makes them (init + a `noise` perturbation) and `rows` random
  configurations."""
  cfgs = vo.random_configurations(n, rows, np.random.RandomState(seed + 10))
  return make_theta(ansatz, n, h, L, seed, noise), cfgs

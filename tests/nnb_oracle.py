"""fp64 restatement of FullyConnectedNNB (wavefunctions.py:931-998) for the tests.

Trunk: h = relu(Linear_H(... relu(Linear_H(x)) ...)) with L hidden layers, out = Linear_{N^2}(h); F(x) =
out.reshape(N, N); psi(x) = det M(x), M[r][c] = F(x)[U_r][D_c] over the up sites U and the down sites D of x in ascending
order.  logit = ln|det M|, psi = sign(det M) exp(logit): no exponent shift.  d ln|psi| / d out[U_r N + D_c] =
(M^-1)[c][r], zero for the other outputs; that row is back-propagated through the trunk.  theta is the flat vector
w_1 [N,H], b_1 [H], (w_l [H,H], b_l [H]) x (L-1), w_out [H,N^2], b_out [N^2].  The sampler, the Hamiltonian and the
accumulator formulas come from oracle.vmc_oracle through an amp_fn.
"""
import numpy as np

from oracle import vmc_oracle as vo


def num_params(n, num_layers, h):
  return n * h + h + (num_layers - 1) * (h * h + h) + h * n * n + n * n


def unpack(theta, n, num_layers, h, dtype=np.float64):
  """[(w, b)] of the L + 1 linear layers."""
  theta = np.asarray(theta, dtype)
  assert theta.size == num_params(n, num_layers, h)
  out, off, fan_in = [], 0, n
  for l in range(num_layers + 1):
    width = h if l < num_layers else n * n
    w = theta[off:off + fan_in * width].reshape(fan_in, width); off += fan_in * width
    b = theta[off:off + width]; off += width
    out.append((w, b))
    fan_in = width
  return out


def offsets(n, num_layers, h):
  """(offset of w_out, offset of b_out) in theta."""
  p = num_params(n, num_layers, h)
  return p - n * n - h * n * n, p - n * n


def default_theta(n, num_layers, h, seed):
  """FullyConnectedNetwork.initialize: truncated normal (2 sigma) with sigma = 1/sqrt(fan_in), zero biases."""
  rng = np.random.default_rng(seed)
  parts, fan_in = [], n
  for l in range(num_layers + 1):
    width = h if l < num_layers else n * n
    w = rng.standard_normal((fan_in, width))
    bad = np.abs(w) > 2
    while bad.any():
      w[bad] = rng.standard_normal(int(bad.sum()))
      bad = np.abs(w) > 2
    parts += [(w / np.sqrt(fan_in)).ravel(), np.zeros(width)]
    fan_in = width
  return np.concatenate(parts).astype(np.float32)


def forward(theta, configs, num_layers, h, dtype=np.float64):
  """(activations [x, a_1 .. a_L], out [B, N^2])."""
  x = np.asarray(configs, dtype)
  layers = unpack(theta, x.shape[1], num_layers, h, dtype)
  acts = [x]
  for w, b in layers[:-1]:
    acts.append(np.maximum(acts[-1] @ w + b, 0))
  w, b = layers[-1]
  return acts, acts[-1] @ w + b


def matrices(theta, configs, num_layers, h, dtype=np.float64):
  x = np.asarray(configs)
  n = x.shape[1]
  _, out = forward(theta, x, num_layers, h, dtype)
  ms = []
  for row, o in zip(x, out):
    up, dn = np.flatnonzero(row > 0), np.flatnonzero(row < 0)
    if up.size != dn.size or 2 * up.size != n:
      raise ValueError('nnb rows need as many up as down spins')
    ms.append(o.reshape(n, n)[np.ix_(up, dn)])
  return np.stack(ms)


def logit_sign(theta, configs, num_layers, h, dtype=np.float64):
  """ln|det M| (-inf where singular) and sign(det M) (0 where singular)."""
  sign, logdet = np.linalg.slogdet(matrices(theta, configs, num_layers, h, dtype))
  return logdet, sign


def psi(theta, configs, num_layers, h, dtype=np.float64):
  logit, sign = logit_sign(theta, configs, num_layers, h, dtype)
  with np.errstate(over='ignore'):
    return sign * np.exp(logit)


def amp_fn(theta, num_layers, h):
  return lambda c: psi(theta, c, num_layers, h)


def condition_numbers(theta, configs, num_layers, h):
  s = np.linalg.svd(matrices(theta, configs, num_layers, h), compute_uv=False)
  with np.errstate(divide='ignore'):
    return s[:, 0] / s[:, -1]


def log_derivatives(theta, configs, num_layers, h):
  """O[b, k] = d ln|psi_b| / d theta_k, in the order of theta."""
  x = np.asarray(configs, np.float64)
  bsz, n = x.shape
  layers = unpack(theta, n, num_layers, h)
  acts, out = forward(theta, x, num_layers, h)
  delta = np.zeros((bsz, n * n))
  for r_b, (row, o) in enumerate(zip(x, out)):
    up, dn = np.flatnonzero(row > 0), np.flatnonzero(row < 0)
    inv = np.linalg.inv(o.reshape(n, n)[np.ix_(up, dn)])
    d = np.zeros((n, n))
    d[np.ix_(up, dn)] = inv.T                 # d[U_r, D_c] = inv[c, r]
    delta[r_b] = d.ravel()
  grads = []
  for l in range(num_layers, -1, -1):
    a = acts[l]
    grads.append((a[:, :, None] * delta[:, None, :]).reshape(bsz, -1))     # d / d w_l
    grads.append(delta)                                                    # d / d b_l
    if l > 0:
      delta = (delta @ layers[l][0].T) * (acts[l] > 0)
  # grads holds (w_L, b_L, w_{L-1}, b_{L-1}, ...): reverse pairwise
  ordered = []
  for l in range(num_layers + 1):
    ordered += [grads[2 * (num_layers - l)], grads[2 * (num_layers - l) + 1]]
  return np.concatenate(ordered, axis=1)


def local_energy(theta, configs, bonds, j_x, j_z, num_layers, h):
  return vo.local_value(amp_fn(theta, num_layers, h), np.asarray(configs, np.float32), bonds, j_x, j_z,
                        dtype=np.float64)


def exchange_terms(theta, configs, bonds, j_x, num_layers, h, dtype=np.float64):
  """terms[b, k] = 0.5 jx_k psi(x_b with bond k exchanged) / psi(x_b) for the antiparallel bonds of row b (zero for the
  others) as k_nnb_rows forms them: sign' sign exp(logit' - logit) from the two (logit, sign) pairs.  dtype float32: the
  trunk, the pairing layer, the elimination (pbdg_oracle.eliminate_fp32), the logits and their difference in float32."""
  x = np.asarray(configs, np.float32)
  jx = np.broadcast_to(np.asarray(j_x, dtype), (len(bonds),))

  def amplitudes(rows):
    if dtype is not np.float32:
      return logit_sign(theta, rows, num_layers, h, dtype)
    from tests import pbdg_oracle as po
    res = [po.eliminate_fp32(m)[1:] for m in matrices(theta, rows, num_layers, h, np.float32)]
    return np.array([r[1] for r in res], np.float32), np.array([r[0] for r in res], np.float32)

  l0, s0 = amplitudes(x)
  out = np.zeros((x.shape[0], len(bonds)), dtype)
  for k, (i, j) in enumerate(bonds):
    live = np.flatnonzero(x[:, i] * x[:, j] < 0)
    if live.size:
      new = x[live].copy()
      new[:, [i, j]] = new[:, [j, i]]
      l1, s1 = amplitudes(new)
      out[live, k] = dtype(0.5) * jx[k] * (s1 * s0[live]).astype(dtype) * np.exp((l1 - l0[live]).astype(dtype))
  return out


def energy_gradient_accumulate(acc, theta, configs, bonds, j_x, j_z, num_layers, h):
  """vo.energy_gradient_accumulate (training.py:539-558) on the nnb ansatz, in fp64."""
  e_loc = local_energy(theta, configs, bonds, j_x, j_z, num_layers, h)
  o = log_derivatives(theta, configs, num_layers, h)
  acc.g1_total += o.sum(0); acc.g2_total += (e_loc[:, None] * o).sum(0); acc.g_count += 1
  acc.e_total += e_loc.sum(); acc.e_count += e_loc.size
  return e_loc


def log_overlap_accumulate(acc, theta, theta_omega, configs, bonds, j_x, j_z, beta, num_layers, h):
  """vo.log_overlap_accumulate (training.py:661-695) on the nnb ansatz with signed amplitudes, in fp64."""
  amp, amp_w = amp_fn(theta, num_layers, h), amp_fn(theta_omega, num_layers, h)
  p, p_w = amp(configs), amp_w(configs)
  h_psi_w = vo.apply_in_place(amp_w, configs, bonds, j_x, j_z, p_w, np.float64)
  ratio = (p_w - beta * h_psi_w) / p
  e_loc = h_psi_w / p_w
  o = log_derivatives(theta, configs, num_layers, h)
  acc.g1_total += o.sum(0); acc.g2_total += (ratio[:, None] * o).sum(0); acc.g_count += 1
  acc.e_total += e_loc.sum(); acc.e_count += e_loc.size
  acc.r_total += ratio.sum(); acc.r_count += ratio.size
  return e_loc, ratio


def exact_energy(theta, bonds, j_x, j_z, n, num_layers, h, configs):
  """<psi|H|psi> / <psi|psi> over `configs` (the whole Sz = 0 sector)."""
  p = psi(theta, configs, num_layers, h)
  e_loc = np.zeros(len(configs))
  nz = p != 0
  e_loc[nz] = vo.local_value(amp_fn(theta, num_layers, h), configs[nz], bonds, j_x, j_z, p[nz], np.float64)
  w = p ** 2
  return float((w * e_loc).sum() / w.sum())

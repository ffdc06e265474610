"""fp64 restatement of ProjectedBDG (wavefunctions.py:876-928) for the tests.

psi(x) = det M(x), M[r][c] = F[U_r][D_c] over the up sites U and the down sites D of x in ascending order (the
reference's boolean_mask order), F = theta.reshape(N, N); logit = ln|det M|, psi = sign(det M) exp(logit - shift).
O_ik = d ln|psi| / d F_ik = (M^-1)[c][r] where U_r = i and D_c = k, zero elsewhere.  An exchange of the up site a with
the down site b changes psi by (-1)^(|a-b|-1) det K (exchange_ratio).  The sampler, the Hamiltonian and the
accumulator formulas come from oracle.vmc_oracle through an amp_fn.
"""
import itertools

import numpy as np

from oracle import vmc_oracle as vo


def pairing(theta, n_sites, dtype=np.float64):
  return np.asarray(theta, dtype).reshape(n_sites, n_sites)


def matrices(theta, configs, dtype=np.float64):
  """M(x) of every row: [B, n, n]."""
  x = np.asarray(configs)
  n_sites = x.shape[1]
  f = pairing(theta, n_sites, dtype)
  out = []
  for row in x:
    up, dn = np.flatnonzero(row > 0), np.flatnonzero(row < 0)
    if up.size != dn.size or 2 * up.size != n_sites:
      raise ValueError('pbdg rows need as many up as down spins')
    out.append(f[np.ix_(up, dn)])
  return np.stack(out)


def logit_sign(theta, configs, dtype=np.float64):
  """ln|det M| (-inf where singular) and sign(det M) (0 where singular)."""
  sign, logdet = np.linalg.slogdet(matrices(theta, configs, dtype))
  return logdet, sign


def psi(theta, configs, shift=-10.0, dtype=np.float64):
  logit, sign = logit_sign(theta, configs, dtype)
  with np.errstate(over='ignore'):
    return sign * np.exp(logit - dtype(shift))


def amp_fn(theta, shift=-10.0):
  return lambda c: psi(theta, c, shift)


def condition_numbers(theta, configs):
  s = np.linalg.svd(matrices(theta, configs), compute_uv=False)
  with np.errstate(divide='ignore'):
    return s[:, 0] / s[:, -1]


def log_derivatives(theta, configs):
  """O[b, i*N + k] = d ln|psi_b| / d F_ik."""
  x = np.asarray(configs)
  b, n_sites = x.shape
  out = np.zeros((b, n_sites * n_sites))
  for r_b, (row, m) in enumerate(zip(x, matrices(theta, x))):
    up, dn = np.flatnonzero(row > 0), np.flatnonzero(row < 0)
    inv = np.linalg.inv(m)
    o = np.zeros((n_sites, n_sites))
    o[np.ix_(up, dn)] = inv.T                 # O[U_r, D_c] = inv[c, r]
    out[r_b] = o.ravel()
  return out


def exchange_ratio(theta, config, a, b):
  """psi(x') / psi(x) for the up site a exchanged with the down site b, by the 2 x 2 determinant of the rank-2
  update of M (no factorisation of M')."""
  row = np.asarray(config)
  n_sites = row.size
  f = pairing(theta, n_sites)
  up, dn = np.flatnonzero(row > 0), np.flatnonzero(row < 0)
  r, c = int(np.flatnonzero(up == a)[0]), int(np.flatnonzero(dn == b)[0])
  inv = np.linalg.inv(f[np.ix_(up, dn)])
  x = f[b, dn] - f[a, dn]
  x[c] = f[b, a] - f[a, b]
  y = f[up, a] - f[up, b]
  y[r] = 0.0
  k = np.array([[1.0 + x @ inv[:, r], x @ inv @ y], [inv[c, r], 1.0 + inv[c, :] @ y]])
  return (-1.0) ** (abs(a - b) - 1) * np.linalg.det(k)


def exchange_ratio_direct(theta, config, a, b):
  row = np.array(config, np.float64)
  new = row.copy()
  new[a], new[b] = -1.0, 1.0
  l0, s0 = logit_sign(theta, row[None])
  l1, s1 = logit_sign(theta, new[None])
  return float(s1[0] * s0[0] * np.exp(l1[0] - l0[0]))


def local_energy(theta, configs, bonds, j_x, j_z):
  return vo.local_value(amp_fn(theta), np.asarray(configs, np.float32), bonds, j_x, j_z, dtype=np.float64)


def energy_gradient_accumulate(acc, theta, configs, bonds, j_x, j_z, shift=-10.0):
  """vo.energy_gradient_accumulate (training.py:539-558) on the pbdg ansatz, in fp64."""
  e_loc = vo.local_value(amp_fn(theta, shift), configs, bonds, j_x, j_z, dtype=np.float64)
  o = log_derivatives(theta, configs)
  acc.g1_total += o.sum(0); acc.g2_total += (e_loc[:, None] * o).sum(0); acc.g_count += 1
  acc.e_total += e_loc.sum(); acc.e_count += e_loc.size
  return e_loc


def log_overlap_accumulate(acc, theta, theta_omega, configs, bonds, j_x, j_z, shift, shift_omega, beta):
  """vo.log_overlap_accumulate (training.py:661-695) on the pbdg ansatz with signed amplitudes, in fp64."""
  amp, amp_w = amp_fn(theta, shift), amp_fn(theta_omega, shift_omega)
  p, p_w = amp(configs), amp_w(configs)
  h_psi_w = vo.apply_in_place(amp_w, configs, bonds, j_x, j_z, p_w, np.float64)
  ratio = (p_w - beta * h_psi_w) / p
  e_loc = h_psi_w / p_w
  o = log_derivatives(theta, configs)
  acc.g1_total += o.sum(0); acc.g2_total += (ratio[:, None] * o).sum(0); acc.g_count += 1
  acc.e_total += e_loc.sum(); acc.e_count += e_loc.size
  acc.r_total += ratio.sum(); acc.r_count += ratio.size
  return e_loc, ratio


def sz0_configurations(n_sites):
  """Every configuration with n_sites / 2 up spins (C(16, 8) = 12,870 on 4 x 4)."""
  out = []
  for up in itertools.combinations(range(n_sites), n_sites // 2):
    row = -np.ones(n_sites, np.float32)
    row[list(up)] = 1.0
    out.append(row)
  return np.stack(out)


def exact_energy(theta, bonds, j_x, j_z, n_sites):
  """<psi|H|psi> / <psi|psi> by enumerating the Sz = 0 sector."""
  cfg = sz0_configurations(n_sites)
  p = psi(theta, cfg, 0.0)
  e_loc = np.zeros(len(cfg))
  nz = p != 0
  e_loc[nz] = vo.local_value(amp_fn(theta, 0.0), cfg[nz], bonds, j_x, j_z, p[nz], np.float64)
  w = p ** 2
  return float((w * e_loc).sum() / w.sum())


def update_norm_shift(psi_values, shift, max_value=1e10):
  """Wavefunction.update_norm on signed amplitudes: log(max_b psi_b); the shift is kept when no psi > 0 (B10)."""
  top = np.max(psi_values)
  if not top > 0:
    return shift
  log_max = np.log(top)
  max_log = np.log(max_value)
  return shift + (log_max - max_log) if log_max > max_log else shift

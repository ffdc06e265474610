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


def eliminate_fp32(m):
  """(M^-1, sign(det M), ln|det M|) by Gauss-Jordan elimination with partial pivoting, every operation on the matrix in
  float32 (pb_eliminate's algorithm, without fused multiply-adds); the logarithms of the pivots are summed in double
  and rounded to float32 once, as in the kernel.  numpy.linalg is no stand-in: on a float32 matrix with kappa = 3,000
  its inv returned the inverse to 4e-8 of its largest entry -- the exact inverse rounded once, not a float32
  factorisation, whose error is about a tenth of eps32 kappa."""
  a = np.array(m, np.float32)
  n = len(a)
  perm = []
  sign, logdet = 1.0, 0.0
  for k in range(n):
    p = k + int(np.argmax(np.abs(a[k:, k])))
    perm.append(p)
    if p != k:
      a[[k, p]] = a[[p, k]]
      sign = -sign
    piv = a[k, k]
    if piv == 0:
      return a, 0.0, np.float32(-np.inf)
    sign = -sign if piv < 0 else sign
    logdet += np.log(np.abs(np.float64(piv)))
    ip = np.float32(1.0) / piv
    a[k, k] = 1.0
    a[k] *= ip
    f = a[:, k].copy()
    f[k] = 0.0
    a[:, k] = 0.0
    a[k, k] = ip
    a -= f[:, None] * a[k][None, :]
  for k in range(n - 1, -1, -1):
    if perm[k] != k:
      a[:, [k, perm[k]]] = a[:, [perm[k], k]]
  return a, sign, np.float32(logdet)


def inverse_fp32(m):
  return eliminate_fp32(m)[0]


def _inverse(m):
  return inverse_fp32(m) if m.dtype == np.float32 else np.linalg.inv(m)


def exchange_ratio_fp32(theta, config, a, b):
  """exchange_ratio with F, a fresh inverse (inverse_fp32) and every product of the 2 x 2 determinant in float32: what
  k_pbdg_eloc computes up to its summation order."""
  row = np.asarray(config)
  n_sites = row.size
  f = pairing(theta, n_sites, np.float32)
  up, dn = np.flatnonzero(row > 0), np.flatnonzero(row < 0)
  r, c = int(np.flatnonzero(up == a)[0]), int(np.flatnonzero(dn == b)[0])
  inv = inverse_fp32(f[np.ix_(up, dn)])
  return np.float32((-1.0) ** (abs(a - b) - 1)) * _det_k(f, inv, up, dn, a, b, r, c)[0]


def _det_k(f, inv, up, dn, a, b, r, c):
  """(det K, K, x, M^-1 y) of exchanging the up site a (U slot r) with the down site b (D slot c), in the dtype of f and
  inv; up / dn are the slot lists (any order)."""
  one = f.dtype.type(1.0)
  x = f[b, dn] - f[a, dn]
  x[c] = f[b, a] - f[a, b]
  y = f[up, a] - f[up, b]
  y[r] = 0
  a1 = inv @ y
  k = np.array([[one + x @ inv[:, r], x @ a1], [inv[c, r], one + a1[c]]], f.dtype)
  return k[0, 0] * k[1, 1] - k[0, 1] * k[1, 0], k, x, a1


def refresh_interval(n_sites):
  """plan_pbdg_refresh_interval: accepted moves of a chain between two fresh factorisations."""
  return min(max(n_sites // 2, 16), 128)


TINY_RATIO = 1e-2     # PLAN_PBDG_TINY_RATIO: an accepted move with |det K| below it is followed by a refresh


def sampler_emulation(theta, configs, seed, n_steps):
  """k_pbdg_sweep's algorithm in numpy with the inverse held in float32: a fresh inverse (inverse_fp32, sorted slots) at
  the start, per step the proposal of vo.step_uniforms / vo.propose_exchange, |det K| of the 2 x 2 determinant against
  sqrt(u), the rank-2 update of an accepted move, and a fresh inverse after refresh_interval accepted moves or after
  a move with |det K| < TINY_RATIO.  Summation orders are numpy's, not the kernel's.  Every chain follows its own fp32
  decisions; next to each the fp64 ratio of the same move is recorded as exp of the slogdet logit difference.

  Returns a dict of [n_steps, B] arrays -- rho32, rho64, u, accept, i_up, i_dn, slot_up, slot_dn (the slots of the two
  sites in the sampler's slot order), fresh (no update since the last factorisation) -- and 'configs', the final
  chains."""
  cur = np.array(configs, np.float32)
  bsz, n_sites = cur.shape
  f = pairing(theta, n_sites, np.float32)
  refresh = refresh_interval(n_sites)
  keys = ('rho32', 'rho64', 'u', 'accept', 'i_up', 'i_dn', 'slot_up', 'slot_dn', 'fresh')
  out = {k: np.zeros((n_steps, bsz), {'rho32': np.float32, 'u': np.float32, 'rho64': np.float64, 'accept': bool,
                                      'fresh': bool}.get(k, np.int64)) for k in keys}

  def factor(row):
    up, dn = np.flatnonzero(row > 0), np.flatnonzero(row < 0)
    return up, dn, inverse_fp32(f[np.ix_(up, dn)])

  state = [factor(row) + (0,) for row in cur]
  logit = logit_sign(theta, cur)[0]
  for step in range(n_steps):
    u_sites, u_acc = vo.step_uniforms(seed, np.arange(bsz), step, n_sites)
    i_up, i_dn = vo.propose_exchange(cur, u_sites)
    new = cur.copy()
    rows = np.arange(bsz)
    new[rows, i_up], new[rows, i_dn] = -1.0, 1.0
    logit_new = logit_sign(theta, new)[0]
    for ch in range(bsz):
      up, dn, inv, since = state[ch]
      a, b = int(i_up[ch]), int(i_dn[ch])
      r, c = int(np.flatnonzero(up == a)[0]), int(np.flatnonzero(dn == b)[0])
      det, k, x, a1 = _det_k(f, inv, up, dn, a, b, r, c)
      acc = bool(np.abs(det) > np.sqrt(u_acc[ch]))
      for key, v in (('rho32', np.abs(det)), ('rho64', np.exp(logit_new[ch] - logit[ch])), ('u', u_acc[ch]),
                     ('accept', acc), ('i_up', a), ('i_dn', b), ('slot_up', r), ('slot_dn', c), ('fresh', since == 0)):
        out[key][step, ch] = v
      if not acc:
        continue
      kinv = np.array([[k[1, 1], -k[0, 1]], [-k[1, 0], k[0, 0]]], np.float32) * (np.float32(1.0) / det)
      left = np.stack([inv[:, r], a1], 1)                    # [M^-1[:, r], M^-1 y]
      right = np.stack([x @ inv, inv[c, :]], 0)              # [x^T M^-1; M^-1[c, :]]
      inv = inv - left @ (kinv @ right)
      up, dn = up.copy(), dn.copy()
      up[r], dn[c] = b, a
      cur[ch, a], cur[ch, b] = -1.0, 1.0
      logit[ch] = logit_new[ch]
      since += 1
      if since >= refresh or not np.abs(det) >= np.float32(TINY_RATIO):
        up, dn, inv = factor(cur[ch])
        since = 0
      state[ch] = (up, dn, inv, since)
  out['configs'] = cur
  return out


def exchange_terms(theta, configs, bonds, j_x, dtype=np.float64, flip=None):
  """terms[b, k] = 0.5 jx_k psi(x_b with bond k exchanged) / psi(x_b) for the antiparallel bonds of row b (zero for the
  others), each from a fresh inverse and the 2 x 2 determinant in `dtype` with the parity factor (-1)^(|a-b|-1): the
  route of k_pbdg_eloc.  flip = (b, k) negates that one term (a wrong parity, for the sharpness check)."""
  x = np.asarray(configs)
  n_sites = x.shape[1]
  f = pairing(theta, n_sites, dtype)
  jx = np.broadcast_to(np.asarray(j_x, dtype), (len(bonds),))
  out = np.zeros((x.shape[0], len(bonds)), dtype)
  for r_b, row in enumerate(x):
    up, dn = np.flatnonzero(row > 0), np.flatnonzero(row < 0)
    pos = np.zeros(n_sites, np.int64)
    pos[up], pos[dn] = np.arange(up.size), np.arange(dn.size)
    inv = _inverse(f[np.ix_(up, dn)])
    for k, (i, j) in enumerate(bonds):
      if row[i] * row[j] < 0:
        a, b = (i, j) if row[i] > 0 else (j, i)
        det = _det_k(f, inv, up, dn, a, b, pos[a], pos[b])[0]
        out[r_b, k] = dtype(0.5) * jx[k] * (-det if (abs(a - b) - 1) & 1 else det)
  if flip is not None:
    out[flip] = -out[flip]
  return out


def diagonal_energy(configs, bonds, j_z, dtype=np.float64):
  x = np.asarray(configs, dtype)
  ij = np.asarray(bonds).reshape(-1, 2)
  jz = np.broadcast_to(np.asarray(j_z, dtype), (len(ij),))
  return ((x[:, ij[:, 0]] * x[:, ij[:, 1]]) * (dtype(0.25) * jz)).sum(1, dtype=dtype)


def local_energy_fp32(theta, configs, bonds, j_x, j_z):
  """The local energies as k_pbdg_eloc forms them, in float32 throughout (fresh float32 inverse, float32 sums)."""
  terms = exchange_terms(theta, configs, bonds, j_x, np.float32)
  return diagonal_energy(configs, bonds, j_z, np.float32) + terms.sum(1, dtype=np.float32)


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

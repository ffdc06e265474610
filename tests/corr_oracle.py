"""fp64 numpy restatement of the spin-correlation measurement (vmc_pair_correlations, evaluation.SpinCorrelationEvaluator)
for any `psi(configs) -> amplitudes` callable, plus brute-force <psi|S_i . S_j|psi> from dense spin matrices.

Local values on a configuration x (s = +-1): S_i . S_j psi (x) / psi(x) = s_i s_j / 4 + [s_i s_j < 0] psi(swap_ij x) / (2 psi(x)).
Test infrastructure; nothing here is used by the product path."""
import numpy as np


def pair_terms(psi, configs, pairs):
  """(sz [B][n_pairs] = s_i s_j, ratio [B][n_pairs] = [s_i s_j < 0] psi(swap_ij x) / psi(x)), fp64."""
  cfg = np.asarray(configs, np.float32)
  pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
  p0 = np.asarray(psi(cfg), np.float64)
  sz = np.zeros((len(cfg), len(pairs)))
  ratio = np.zeros((len(cfg), len(pairs)))
  for k, (i, j) in enumerate(pairs):
    sz[:, k] = cfg[:, i].astype(np.float64) * cfg[:, j]
    anti = np.flatnonzero(sz[:, k] < 0)
    if anti.size:
      swapped = cfg[anti].copy()
      swapped[:, [i, j]] = swapped[:, [j, i]]
      with np.errstate(divide='ignore', invalid='ignore'):
        ratio[anti, k] = np.asarray(psi(swapped), np.float64) / p0[anti]
  return sz, ratio


def pair_sums(psi, configs, pairs):
  """(zz_sum, ex_sum) [n_pairs] as vmc_pair_correlations defines them."""
  sz, ratio = pair_terms(psi, configs, pairs)
  return sz.sum(0), ratio.sum(0)


def pair_means(psi, configs, pairs):
  """Batch means (szsz, exchange, ss) [n_pairs]: s_i s_j / 4, the ratio / 2 and their sum."""
  zz, ex = pair_sums(psi, configs, pairs)
  b = float(len(configs))
  return 0.25 * zz / b, 0.5 * ex / b, (0.25 * zz + 0.5 * ex) / b


def all_configurations(n):
  """Every +-1 configuration of n sites [2^n][n]; row w has s_i = +1 where bit i of w is set."""
  w = np.arange(1 << n)
  return np.where((w[:, None] >> np.arange(n)) & 1, 1.0, -1.0).astype(np.float32)


def vector_psi(vector):
  """psi(configs) that looks the amplitudes up in a vector over all_configurations (bit i set: s_i = +1)."""
  vec = np.asarray(vector, np.float64)

  def psi(configs):
    cfg = np.asarray(configs)
    return vec[(cfg > 0).astype(np.int64) @ (1 << np.arange(cfg.shape[1]))]
  return psi


def expectation(psi, configs, pairs):
  """sum_x |psi(x)|^2 local(x) / sum_x |psi(x)|^2 over `configs` (the whole basis: the exact <S_i . S_j>); configurations
  with psi = 0 carry no weight."""
  cfg = np.asarray(configs, np.float32)
  p = np.asarray(psi(cfg), np.float64)
  keep = p != 0
  sz, ratio = pair_terms(psi, cfg[keep], pairs)
  w = p[keep] ** 2
  return (w[:, None] * (0.25 * sz + 0.5 * ratio)).sum(0) / w.sum()


def dense_ss_matrix(n, i, j):
  """S_i . S_j as a dense [2^n][2^n] matrix in the basis of all_configurations (site 0 = the lowest bit)."""
  sx = np.array([[0.0, 0.5], [0.5, 0.0]])
  sy = np.array([[0.0, -0.5j], [0.5j, 0.0]])
  sz = np.array([[-0.5, 0.0], [0.0, 0.5]])           # index 1 = bit set = spin up

  def site_op(op, site):
    out = np.eye(1)
    for s in range(n - 1, -1, -1):                    # the highest site is the slowest index
      out = np.kron(out, op if s == site else np.eye(2))
    return out
  m = sum(site_op(o, i) @ site_op(o, j) for o in (sx, sy, sz))
  assert np.abs(m.imag).max() == 0
  return m.real


def neel_configuration(coords):
  """+-1 by the parity of the summed integer coordinates (the chain: alternating; the torus: checkerboard)."""
  c = np.asarray(coords).reshape(len(coords), -1)
  return np.where(np.rint(c).astype(np.int64).sum(1) % 2 == 0, 1.0, -1.0).astype(np.float32)

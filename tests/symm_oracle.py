"""fp64 numpy restatement of the symmetry expectation values (vmc_symmetry_expectations, evaluation.SymmetryEvaluator)
for any `psi(configs) -> amplitudes` callable, plus the exact expectation of an op over an explicit Sz = 0 vector.

An op is a site permutation `perm`, optionally followed by the global spin flip: row[i] = f x[perm[i]], f = -1 with the
flip.  A chain's term is psi(row) / psi(x), 0 where either amplitude vanishes; <P> is the mean of the terms over chains
drawn from |psi|^2.  Test infrastructure; nothing here is used by the product path."""
import numpy as np


def rows(configs, perm, flip):
  """[B][N] float32: row[c][i] = f configs[c][perm[i]]."""
  cfg = np.asarray(configs, np.float32)
  out = cfg[:, np.asarray(perm, np.int64)]
  return -out if flip else out


def terms(psi, configs, perms, flips=None):
  """[n_ops][B] fp64: psi(row_{k,c}) / psi(x_c), 0 where either amplitude vanishes."""
  cfg = np.asarray(configs, np.float32)
  perms = np.asarray(perms, np.int64).reshape(-1, cfg.shape[1])
  flips = np.zeros(len(perms), np.int64) if flips is None else np.asarray(flips, np.int64).ravel()
  own = np.asarray(psi(cfg), np.float64)
  out = np.zeros((len(perms), len(cfg)))
  for k, (perm, flip) in enumerate(zip(perms, flips)):
    num = np.asarray(psi(rows(cfg, perm, flip)), np.float64)
    ok = (num != 0) & (own != 0)
    out[k, ok] = num[ok] / own[ok]
  return out


def sums(psi, configs, perms, flips=None):
  """ratio_sum [n_ops] as vmc_symmetry_expectations defines it (any fixed order: the bound of the GPU test covers it)."""
  return terms(psi, configs, perms, flips).sum(1)


def exact_expectation(vector, basis, index, perm, flip):
  """<v| P |v> / <v|v> over a full Sz = 0 vector: `basis` [D][N] are its configurations, index(configs) -> their
  positions in `vector`; (P v)(x) = v(row(x))."""
  vec = np.asarray(vector, np.float64)
  cfg = np.asarray(basis, np.float32)
  own = vec[index(cfg)]
  moved = vec[index(rows(cfg, perm, flip))]
  return float((own * moved).sum() / (own * own).sum())

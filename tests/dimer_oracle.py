"""fp64 numpy restatement of the dimer-dimer estimator (vmc_dimer_correlations, evaluation.DimerCorrelationEvaluator) for
any `psi(configs) -> amplitudes` callable, plus the exact <psi| (S_i . S_j)(S_k . S_l) |psi> of an explicit vector over
the Sz = 0 basis by applying the two operators to the vector.

With a = (i, j), b = (k, l), r(y) = psi(y) / psi(x), x' = swap_ij x and s' the spins of x':
  bond(a; x)  = s_i s_j / 4 + [s_i != s_j] r(x') / 2
  dd(a, b; x) = s_i s_j / 4 (s_k s_l / 4 + [s_k != s_l] r(swap_kl x) / 2)
              + [s_i != s_j] / 2 (s'_k s'_l r(x') / 4 + [s'_k != s'_l] r(swap_kl x') / 2)
A vanishing amplitude of an exchanged configuration gives the ratio 0; a chain whose own amplitude vanishes gives 0 for
every value.  Test infrastructure; nothing here is used by the product path."""
import numpy as np


def exchanged(configs, i, j):
  """A copy of `configs` with the spins of sites i and j exchanged in every row."""
  out = np.array(configs, np.float32, copy=True)
  out[:, [i, j]] = out[:, [j, i]]
  return out


def _ratios(psi, rows, use, own):
  """psi(rows) / own where `use` holds and both amplitudes are non-zero, else 0; fp64 [B]."""
  r = np.zeros(len(rows))
  idx = np.flatnonzero(use & (own != 0))
  if idx.size:
    num = np.asarray(psi(rows[idx]), np.float64)
    r[idx] = np.where(num != 0, num / own[idx], 0.0)
  return r


def bond_parts(psi, configs, bond, own=None):
  """The pieces of bond(a; x) per chain: dict of zz = s_i s_j / 4, anti = [s_i != s_j], rows = swap_ij x, r = r(rows)
  (0 where not anti), alive = [psi(x) != 0], value = the local value."""
  cfg = np.asarray(configs, np.float32)
  own = np.asarray(psi(cfg), np.float64) if own is None else own
  i, j = int(bond[0]), int(bond[1])
  zz = 0.25 * cfg[:, i].astype(np.float64) * cfg[:, j]
  anti = cfg[:, i] != cfg[:, j]
  rows = exchanged(cfg, i, j)
  r = _ratios(psi, rows, anti, own)
  alive = own != 0
  return dict(zz=zz, anti=anti, rows=rows, r=r, alive=alive, value=np.where(alive, zz + 0.5 * r, 0.0))


def dd_parts(psi, configs, bond_a, bond_b, own=None):
  """The pieces of dd(a, b; x) per chain.  Keys: zz_a, anti_a, rows_a (= x'), r_a; zz_b, anti_b, rows_b (= swap_kl x), r_b
  (B on x); zz_b1 = s'_k s'_l / 4, anti_b1 = [s_i != s_j][s'_k != s'_l], rows_ab = swap_kl x', r_ab (B on x'); alive; terms
  [4][B], the four products the value is the sum of; value."""
  cfg = np.asarray(configs, np.float32)
  own = np.asarray(psi(cfg), np.float64) if own is None else own
  a = bond_parts(psi, cfg, bond_a, own)
  b = bond_parts(psi, cfg, bond_b, own)
  k, l = int(bond_b[0]), int(bond_b[1])
  xp = a['rows']                                                   # x' where anti_a holds (unused elsewhere)
  zz_b1 = 0.25 * xp[:, k].astype(np.float64) * xp[:, l]
  anti_b1 = a['anti'] & (xp[:, k] != xp[:, l])
  rows_ab = exchanged(xp, k, l)
  r_ab = _ratios(psi, rows_ab, anti_b1, own)
  alive = own != 0
  terms = np.stack([a['zz'] * b['zz'], a['zz'] * 0.5 * b['r'], 0.5 * zz_b1 * a['r'], 0.25 * r_ab]) * alive
  return dict(zz_a=a['zz'], anti_a=a['anti'], rows_a=xp, r_a=a['r'], zz_b=b['zz'], anti_b=b['anti'], rows_b=b['rows'],
              r_b=b['r'], zz_b1=zz_b1, anti_b1=anti_b1, rows_ab=rows_ab, r_ab=r_ab, alive=alive, terms=terms,
              value=terms.sum(0))


def bond_values(psi, configs, bonds):
  """[n_bonds][B] local values of S_i . S_j."""
  cfg = np.asarray(configs, np.float32)
  own = np.asarray(psi(cfg), np.float64)
  return np.array([bond_parts(psi, cfg, b, own)['value'] for b in bonds]).reshape(len(bonds), len(cfg))


def dd_values(psi, configs, bonds, pairs):
  """[n_pairs][B] local values of (S_i . S_j)(S_k . S_l) for the pairs (a, b) of indices into `bonds`."""
  cfg = np.asarray(configs, np.float32)
  own = np.asarray(psi(cfg), np.float64)
  return np.array([dd_parts(psi, cfg, bonds[a], bonds[b], own)['value'] for a, b in pairs]).reshape(len(pairs), len(cfg))


def ascending_sums(values):
  out = np.zeros(len(values))
  for n, row in enumerate(values):
    s = 0.0
    for t in row:
      s += t
    out[n] = s
  return out


def dimer_sums(psi, configs, bonds, pairs):
  """(bond_sum [n_bonds], dd_sum [n_pairs]) as vmc_dimer_correlations defines them (chains added in ascending order)."""
  return ascending_sums(bond_values(psi, configs, bonds)), ascending_sums(dd_values(psi, configs, bonds, pairs))


def _words(configs):
  bits = (np.asarray(configs) > 0).astype(np.int64)
  return bits @ (1 << np.arange(bits.shape[1], dtype=np.int64))


def apply_bond(vec, basis, bond):
  """(S_i . S_j) v over the configurations `basis` [D][N] (the whole Sz = 0 sector, each once): diagonal s_i s_j / 4,
  and 1 / 2 between a configuration with antiparallel (i, j) and its exchange."""
  cfg = np.asarray(basis, np.float32)
  vec = np.asarray(vec, np.float64)
  i, j = int(bond[0]), int(bond[1])
  words = _words(cfg)
  order = np.argsort(words)
  out = 0.25 * cfg[:, i].astype(np.float64) * cfg[:, j] * vec
  anti = np.flatnonzero(cfg[:, i] != cfg[:, j])
  partner = order[np.searchsorted(words[order], _words(exchanged(cfg[anti], i, j)))]
  out[anti] += 0.5 * vec[partner]
  return out


def exact_bond(vec, basis, bond):
  vec = np.asarray(vec, np.float64)
  return float(vec @ apply_bond(vec, basis, bond) / (vec @ vec))


def exact_dd(vec, basis, bond_a, bond_b):
  """<v| A B |v> / <v|v> = (A v) . (B v) / v . v (A is symmetric): no intermediate configuration, no ratio."""
  vec = np.asarray(vec, np.float64)
  return float(apply_bond(vec, basis, bond_a) @ apply_bond(vec, basis, bond_b) / (vec @ vec))

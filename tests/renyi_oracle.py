"""fp64 numpy restatement of the replica swap estimator of the second Renyi entropy (vmc_renyi2_swap,
evaluation.RenyiEntropyEvaluator) for any `psi(configs) -> amplitudes` callable, plus the exact Tr rho_A^2 of an explicit
Sz = 0 vector by singular values.

The chains are the B / 2 replica pairs (c, c + B / 2).  For a region A (a 0/1 mask over the sites) a pair MATCHES when both
chains hold the same sum of spins on A; its term is psi(x~) psi(y~) / (psi(x) psi(y)) with the spins of A exchanged between
the two, any other pair's term is 0 (the swapped configurations would leave the Sz = 0 sector), and so is the term of a pair
with a vanishing amplitude among the four.  Test infrastructure; nothing here is used by the product path."""
import numpy as np


def masks(regions, n_sites):
  """[n_regions][n_sites] bool from a list of site lists."""
  out = np.zeros((len(regions), n_sites), bool)
  for k, region in enumerate(regions):
    out[k, list(region)] = True
  return out


def swap_terms(psi, x, y, mask):
  """(terms [P], match [P] bool) of the pairs (x[p], y[p]) for ONE region mask [N]."""
  x = np.asarray(x, np.float32)
  y = np.asarray(y, np.float32)
  mask = np.asarray(mask, bool)
  match = x[:, mask].astype(np.int64).sum(1) == y[:, mask].astype(np.int64).sum(1)
  terms = np.zeros(len(x))
  idx = np.flatnonzero(match)
  if idx.size:
    xs, ys = x[idx].copy(), y[idx].copy()
    xs[:, mask] = y[idx][:, mask]
    ys[:, mask] = x[idx][:, mask]
    num = np.asarray(psi(xs), np.float64) * np.asarray(psi(ys), np.float64)
    den = np.asarray(psi(x[idx]), np.float64) * np.asarray(psi(y[idx]), np.float64)
    ok = (num != 0) & (den != 0)
    t = np.zeros(idx.size)
    t[ok] = num[ok] / den[ok]
    terms[idx] = t
  return terms, match


def pair_terms(psi, configs, region_masks):
  """(terms [n_regions][B / 2], match [n_regions][B / 2]) over the replica pairs (c, c + B / 2) of `configs`."""
  cfg = np.asarray(configs, np.float32)
  assert len(cfg) % 2 == 0
  half = len(cfg) // 2
  region_masks = np.asarray(region_masks, bool)
  terms = np.zeros((len(region_masks), half))
  match = np.zeros((len(region_masks), half), bool)
  for k, m in enumerate(region_masks):
    terms[k], match[k] = swap_terms(psi, cfg[:half], cfg[half:], m)
  return terms, match


def swap_sums(psi, configs, region_masks):
  """(swap_sum, match_count) [n_regions] as vmc_renyi2_swap defines them (pairs added in ascending order)."""
  terms, match = pair_terms(psi, configs, region_masks)
  sums = np.zeros(len(terms))
  for k in range(len(terms)):
    s = 0.0
    for t in terms[k]:
      s += t
    sums[k] = s
  return sums, match.sum(1).astype(np.float64)


def exact_purity(psi, basis, mask):
  """Tr rho_A^2 of the state whose amplitudes on the configurations `basis` [D][N] (every configuration that carries
  weight, each once) are psi(basis): the amplitudes reshaped to [configurations of A][configurations of the rest] and the
  fourth powers of the singular values of that matrix, normalised."""
  cfg = np.asarray(basis, np.float32)
  mask = np.asarray(mask, bool)
  amp = np.asarray(psi(cfg), np.float64)
  bits = (cfg > 0).astype(np.int64)
  ka = bits[:, mask] @ (1 << np.arange(int(mask.sum())))
  kb = bits[:, ~mask] @ (1 << np.arange(int((~mask).sum())))
  ua, ia = np.unique(ka, return_inverse=True)
  ub, ib = np.unique(kb, return_inverse=True)
  m = np.zeros((len(ua), len(ub)))
  m[ia, ib] = amp
  s = np.linalg.svd(m, compute_uv=False)
  return float((s ** 4).sum() / (s ** 2).sum() ** 2)


def exact_swap_expectation(psi, basis, mask):
  """sum over ALL ordered pairs (x, y) of `basis` of |psi(x)|^2 |psi(y)|^2 term(x, y) / (sum |psi|^2)^2: what the estimator
  averages to.  Equals exact_purity."""
  cfg = np.asarray(basis, np.float32)
  amp = np.asarray(psi(cfg), np.float64)
  w = amp ** 2
  d = len(cfg)
  total = 0.0
  for a in range(d):
    if w[a] == 0:
      continue
    x = np.repeat(cfg[a:a + 1], d, axis=0)
    terms, _ = swap_terms(psi, x, cfg, mask)
    total += w[a] * (w * terms).sum()
  return total / w.sum() ** 2

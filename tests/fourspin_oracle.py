"""fp64 numpy restatement of the four-spin (J-Q) terms (vmc_set_four_spin_terms, operators.JQHamiltonian) for any
`psi(configs) -> amplitudes` callable, plus the sparse matrix of H_J + H_Q over the Sz = 0 basis and its lowest states.

A term t = (i, j, k, l; q_t) with four distinct sites is -q_t (1/4 - S_i . S_j)(1/4 - S_k . S_l).  On spins +-1
(1/4 - S_i . S_j) |x> = [s_i != s_j] (|x> - sigma |swap_ij x>) / 2, sigma = +1 in the physical frame and -1 in the
sublattice-rotated frame that goes with j_x < 0, so with r(y) = psi(y) / psi(x)
  e_t(x) = -(q_t / 4) [s_i != s_j][s_k != s_l] (1 - sigma r(swap_ij x) - sigma r(swap_kl x) + r(swap_kl swap_ij x)).
A vanishing amplitude of an exchanged configuration gives the ratio 0; a chain whose own amplitude vanishes gives 0 for
every value (the library adds nothing to such a chain).  Test infrastructure; nothing here is used by the product path."""
import fractions
import itertools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def exchanged(configs, i, j):
  """A copy of `configs` with the spins of sites i and j exchanged in every row."""
  out = np.array(configs, np.float32, copy=True)
  out[:, [i, j]] = out[:, [j, i]]
  return out


def pair_table(terms):
  """(pairs [n_pairs][2], term_pairs [n_terms][2]): the distinct unordered site pairs (min, max) of the terms, ascending,
  and per term the indices of (i, j) and (k, l) into them -- the table the library reduces the terms to."""
  terms = np.asarray(terms, np.int64).reshape(-1, 4)
  halves = np.sort(terms.reshape(-1, 2), axis=1)
  pairs = sorted({(int(a), int(b)) for a, b in halves})
  index = {p: k for k, p in enumerate(pairs)}
  term_pairs = np.array([index[(int(a), int(b))] for a, b in halves], np.int64).reshape(-1, 2)
  return np.array(pairs, np.int64), term_pairs


def _ratios(psi, rows, use, own):
  """psi(rows) / own where `use` holds and both amplitudes are non-zero, else 0; fp64 [B]."""
  r = np.zeros(len(rows))
  idx = np.flatnonzero(use & (own != 0))
  if idx.size:
    num = np.asarray(psi(rows[idx]), np.float64)
    r[idx] = np.where(num != 0, num / own[idx], 0.0)
  return r


def term_parts(psi, configs, terms, q, sigma, own=None):
  """The pieces of the term sums per chain.  Keys: pairs, term_pairs (pair_table); anti [n_pairs][B]; rows1 (list per pair:
  swap x), r1 [n_pairs][B] (0 where not anti); active [n_terms][B]; rows2 (list per term: the double exchange), r2
  [n_terms][B]; w [n_terms] = -q / 4; alive [B]; products [n_terms][4][B] = w, -sigma w r_ij, -sigma w r_kl, w r_ijkl where
  the term is active and the chain alive; value [n_terms][B]."""
  cfg = np.asarray(configs, np.float32)
  own = np.asarray(psi(cfg), np.float64) if own is None else own
  terms = np.asarray(terms, np.int64).reshape(-1, 4)
  w = -0.25 * np.broadcast_to(np.asarray(q, np.float32), (len(terms),)).astype(np.float64)
  pairs, term_pairs = pair_table(terms)
  alive = own != 0
  anti = np.array([cfg[:, i] != cfg[:, j] for i, j in pairs]).reshape(len(pairs), len(cfg))
  rows1 = [exchanged(cfg, i, j) for i, j in pairs]
  r1 = np.array([_ratios(psi, rows, a, own) for rows, a in zip(rows1, anti)]).reshape(len(pairs), len(cfg))
  active = anti[term_pairs[:, 0]] & anti[term_pairs[:, 1]]
  rows2 = [exchanged(exchanged(cfg, i, j), k, l) for i, j, k, l in terms]
  r2 = np.array([_ratios(psi, rows, a, own) for rows, a in zip(rows2, active)]).reshape(len(terms), len(cfg))
  on = (active & alive).astype(np.float64)
  products = np.stack([w[:, None] * on, -sigma * w[:, None] * r1[term_pairs[:, 0]] * on,
                       -sigma * w[:, None] * r1[term_pairs[:, 1]] * on, w[:, None] * r2 * on], axis=1)
  return dict(pairs=pairs, term_pairs=term_pairs, anti=anti, rows1=rows1, r1=r1, active=active, rows2=rows2, r2=r2, w=w,
              alive=alive, products=products, value=products.sum(1))


def term_sums(psi, configs, terms, q, sigma):
  """[B] sum_t e_t(x_c)."""
  return term_parts(psi, configs, terms, q, sigma)['value'].sum(0)


def row_counts(configs, terms):
  """(single rows, double rows) of the library's list on these chains: they depend on the configurations alone."""
  cfg = np.asarray(configs, np.float32)
  pairs, term_pairs = pair_table(terms)
  anti = np.array([cfg[:, i] != cfg[:, j] for i, j in pairs]).reshape(len(pairs), len(cfg))
  return int(anti.sum()), int((anti[term_pairs[:, 0]] & anti[term_pairs[:, 1]]).sum())


def heisenberg_local(psi, configs, bonds, j_x, j_z, own=None):
  """[B] local energies of sum_bonds (j_z / 4 s_i s_j + j_x / 2 [s_i != s_j] r(swap_ij x)); 0 on a chain that is not alive."""
  cfg = np.asarray(configs, np.float32)
  own = np.asarray(psi(cfg), np.float64) if own is None else own
  jx = np.broadcast_to(np.asarray(j_x, np.float64), (len(bonds),))
  jz = np.broadcast_to(np.asarray(j_z, np.float64), (len(bonds),))
  out = np.zeros(len(cfg))
  for (i, j), x, z in zip(bonds, jx, jz):
    out += 0.25 * z * cfg[:, i].astype(np.float64) * cfg[:, j]
    if x != 0:
      out += 0.5 * x * _ratios(psi, exchanged(cfg, i, j), cfg[:, i] != cfg[:, j], own)
  return np.where(own != 0, out, 0.0)


def local_energy(psi, configs, bonds, j_x, j_z, terms, q, sigma):
  """[B] local energies of H_J + H_Q."""
  cfg = np.asarray(configs, np.float32)
  own = np.asarray(psi(cfg), np.float64)
  return heisenberg_local(psi, cfg, bonds, j_x, j_z, own) + term_parts(psi, cfg, terms, q, sigma, own)['value'].sum(0)


# ---- the fold in the library's own order, from amplitudes given as (ln|psi|, sign) in the library's fp32 bits

def fma(a, b, c):
  """The correctly rounded a b + c of three doubles (exact rational arithmetic, one rounding)."""
  return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


def butterfly(lanes):
  """The xor butterfly 32, 16, ..., 1 over 64 fp64 lanes: what every lane holds at the end."""
  v = np.array(lanes, np.float64)
  assert v.shape == (64,)
  o = 32
  while o > 0:
    v = v + v[np.arange(64) ^ o]
    o >>= 1
  assert (v == v[0]).all()
  return float(v[0])


def ratio_from_logs(row_logit, row_sign, own_logit, own_sign):
  """sgn exp((double) ln|psi(row)| - (double) ln|psi(x)|) from fp32 logs and signs; 0 where the row's amplitude vanishes."""
  sg = np.sign(own_sign) * np.sign(row_sign)
  return 0.0 if sg == 0 else float(sg * np.exp(np.float64(np.float32(row_logit)) - np.float64(np.float32(own_logit))))


def fold_chain(active, w, r_ij, r_kl, r_ijkl, sigma):
  """The fp64 sum of one chain in the documented order: lane l walks the terms l, l + 64, ... ascending; per active term
  it adds w, then fma(-sigma w, r_ij, .), fma(-sigma w, r_kl, .), fma(w, r_ijkl, .); then the butterfly."""
  lanes = [0.0] * 64
  for t in range(len(active)):
    if not active[t]:
      continue
    s = lanes[t % 64]
    s = s + float(w[t])
    s = fma(-sigma * float(w[t]), float(r_ij[t]), s)
    s = fma(-sigma * float(w[t]), float(r_kl[t]), s)
    s = fma(float(w[t]), float(r_ijkl[t]), s)
    lanes[t % 64] = s
  return butterfly(lanes)


# ---- exact diagonalisation of H_J + H_Q

def sz0_basis(n):
  """[C(n, n / 2)][n] fp64 configurations, in the order of tests/exact_states.ed_ground_state."""
  combos = list(itertools.combinations(range(n), n // 2))
  cfgs = np.ones((len(combos), n), np.float64)
  for k, c in enumerate(combos):
    cfgs[k, list(c)] = -1
  return cfgs


def _words(configs):
  bits = (np.asarray(configs) > 0).astype(np.int64)
  return bits @ (1 << np.arange(bits.shape[1], dtype=np.int64))


class Lookup:
  """index / amplitude of configurations in a basis (each configuration once)."""

  def __init__(self, basis):
    self.words = _words(basis)
    self.order = np.argsort(self.words)
    self.sorted = self.words[self.order]

  def index(self, configs):
    w = _words(configs)
    at = np.searchsorted(self.sorted, w)
    assert (self.sorted[at] == w).all()
    return self.order[at]

  def psi(self, vec):
    vec = np.asarray(vec, np.float64)
    return lambda configs: vec[self.index(configs)]


def jq_matrix(basis, bonds, j_x, j_z, terms, q, sigma):
  """H_J + H_Q as a csr matrix over `basis`, from the operators' action on basis states (no local values, no ratios)."""
  cfg = np.asarray(basis, np.float32)
  look = Lookup(cfg)
  dim = len(cfg)
  every = np.arange(dim)
  diag = np.zeros(dim)
  rows, cols, vals = [], [], []

  def add(src, rows_cfg, value):
    rows.append(src); cols.append(look.index(rows_cfg)); vals.append(np.full(len(src), value))
  jx = np.broadcast_to(np.asarray(j_x, np.float64), (len(bonds),))
  jz = np.broadcast_to(np.asarray(j_z, np.float64), (len(bonds),))
  for (i, j), x, z in zip(bonds, jx, jz):
    diag += 0.25 * z * cfg[:, i].astype(np.float64) * cfg[:, j]
    anti = every[cfg[:, i] != cfg[:, j]]
    add(anti, exchanged(cfg[anti], i, j), 0.5 * x)
  terms = np.asarray(terms, np.int64).reshape(-1, 4)
  qs = np.broadcast_to(np.asarray(q, np.float64), (len(terms),))
  for (i, j, k, l), qt in zip(terms, qs):
    act = every[(cfg[:, i] != cfg[:, j]) & (cfg[:, k] != cfg[:, l])]
    w = -0.25 * qt
    diag[act] += w
    add(act, exchanged(cfg[act], i, j), -sigma * w)
    add(act, exchanged(cfg[act], k, l), -sigma * w)
    add(act, exchanged(exchanged(cfg[act], i, j), k, l), w)
  rows.append(every); cols.append(every); vals.append(diag)
  return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(dim, dim))


def jq_lowest(n, bonds, j_x, j_z, terms, q, sigma, k=1):
  """(energies [k] ascending, vectors [dim][k], basis [dim][n], H) of the k lowest states in the Sz = 0 sector."""
  basis = sz0_basis(n)
  hmat = jq_matrix(basis, bonds, j_x, j_z, terms, q, sigma)
  assert abs(hmat - hmat.T).max() < 1e-14
  w, v = spla.eigsh(hmat, k=k, which='SA', tol=1e-13, v0=np.ones(len(basis)))
  order = np.argsort(w)
  return w[order], v[:, order], basis, hmat

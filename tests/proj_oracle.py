"""fp64 numpy restatement of the symmetry-projected energies (vmc_projected_energy, evaluation.ProjectedEnergyEvaluator)
on tests/symm_oracle.py's rows and terms, the exact enumeration of the same estimator over an explicit Sz = 0 vector, and
the bound of the GPU parity tests.

With the ops g_k of symm_oracle (row[i] = f x[perm[i]]), characters chi[s][k] and r_{k,c} = psi(row_{k,c}) / psi(x_c):
  w_s(c) = sum_k chi[s][k] r_{k,c}      w_sum[s] = sum_c w_s(c)      we_sum[s] = sum_c w_s(c) E_loc(c)
A chain whose own amplitude vanishes adds nothing to any sum.  Test infrastructure; nothing here is used by the product
path."""
import numpy as np

from tests import symm_oracle as so


def chain_weights(psi, configs, perms, flips, chi):
  """(w [n_sectors][B], |w| bound pieces a [n_sectors][B] = sum_k |chi[s][k]| |r_{k,c}|, terms [n_ops][B])."""
  terms = so.terms(psi, configs, perms, flips)
  chi = np.asarray(chi, np.float64).reshape(-1, len(terms))
  return chi @ terms, np.abs(chi) @ np.abs(terms), terms


def sums(psi, eloc, configs, perms, flips, chi):
  """dict w_sum, we_sum [n_sectors], e_sum, n_alive as vmc_projected_energy defines them; eloc [B] fp64 (entries of
  chains whose own amplitude vanishes are not read)."""
  cfg = np.asarray(configs, np.float32)
  alive = np.asarray(psi(cfg), np.float64) != 0
  w = chain_weights(psi, cfg, perms, flips, chi)[0]
  e = np.where(alive, np.asarray(eloc, np.float64), 0.0)
  return {'w_sum': w[:, alive].sum(1), 'we_sum': (w[:, alive] * e[alive]).sum(1), 'e_sum': float(e[alive].sum()),
          'n_alive': int(alive.sum())}


def bounds(psi, eps, eloc, d_eloc, configs, perms, flips, chi):
  """(bound of w_sum [n_sectors], bound of we_sum [n_sectors], bound of e_sum).  eps(configs) bounds the error of ln|psi|
  per row (the family's own amplitude parity test), d_eloc [B] that of E_loc per chain (the family's own local-energy
  parity test).  tests/test_gpu_symm.py bounds the sum of op k over the chains, t_kc = r_kc of the oracle, by
    b_k = sum_c |t_kc| (exp(eps(row_kc) + eps(x_c)) - 1) + B 2^-53 sum_c |t_kc|
  and the sums here are linear in those terms:
    |w_sum[s] - ref|  <= sum_k |chi[s][k]| b_k
    |we_sum[s] - ref| <= sum_k |chi[s][k]| b_k(|E_loc|) + sum_c |w_s(c)| dE_c + (B + 1) 2^-53 sum_c |w_s(c)| |E_c|
  with b_k(|E_loc|) the same figure with |E_c| carried through both of its sums (the chains' terms weighted by the
  reference's |E_loc|), the second piece what the local energies' own tolerance admits, the third the fp64 fold of B
  products (one rounding each, hence B + 1).  |e_sum - ref| <= sum_c dE_c + B 2^-53 sum_c |E_c|."""
  cfg = np.asarray(configs, np.float32)
  alive = np.asarray(psi(cfg), np.float64) != 0
  perms = np.asarray(perms, np.int64).reshape(-1, cfg.shape[1])
  flips = np.zeros(len(perms), np.int64) if flips is None else np.asarray(flips, np.int64).ravel()
  w, _, terms = chain_weights(psi, cfg, perms, flips, chi)
  chi = np.asarray(chi, np.float64).reshape(-1, len(terms))
  b, u = len(cfg), 2.0 ** -53
  e_own = eps(cfg)
  rel = np.stack([np.expm1(eps(so.rows(cfg, perm, flip)) + e_own) for perm, flip in zip(perms, flips)])
  e = np.where(alive, np.abs(np.asarray(eloc, np.float64)), 0.0)
  de = np.where(alive, np.asarray(d_eloc, np.float64), 0.0)
  a = np.abs(terms)                                                            # [n_ops][B]; 0 where either amplitude vanishes
  per_op = (a * rel).sum(1) + b * u * a.sum(1)
  per_op_e = (a * rel * e).sum(1) + b * u * (a * e).sum(1)
  aw = np.abs(w) * alive
  w_bound = np.abs(chi) @ per_op
  we_bound = np.abs(chi) @ per_op_e + (aw * de).sum(1) + (b + 1) * u * (aw * e).sum(1)
  e_bound = de.sum() + b * u * e.sum()
  return w_bound, we_bound, e_bound


# ---- exact enumeration over a full Sz = 0 vector

def lookup(basis):
  """index(configs) -> positions in `basis` [D][N] (+-1 rows)."""
  table = {np.asarray(row > 0, np.uint8).tobytes(): i for i, row in enumerate(np.asarray(basis))}
  return lambda cfg: np.array([table[np.asarray(row > 0, np.uint8).tobytes()] for row in np.asarray(cfg)], np.int64)


def hamiltonian_matrix(basis, bonds, j_x, j_z):
  """Dense sum_b j_z Sz Sz + j_x / 2 (S+ S- + h.c.) on `basis`; j_x / j_z one value or one per bond."""
  basis = np.asarray(basis, np.float64)
  index = lookup(basis)
  nb = len(bonds)
  jx, jz = np.broadcast_to(np.asarray(j_x, np.float64), (nb,)), np.broadcast_to(np.asarray(j_z, np.float64), (nb,))
  h = np.zeros((len(basis), len(basis)))
  rows = np.arange(len(basis))
  for (i, j), x, z in zip(bonds, jx, jz):
    h[rows, rows] += 0.25 * z * basis[:, i] * basis[:, j]
    anti = np.flatnonzero(basis[:, i] * basis[:, j] < 0)
    moved = basis[anti].copy()
    moved[:, [i, j]] = moved[:, [j, i]]
    np.add.at(h, (anti, index(moved)), 0.5 * x)
  return h


def op_matrices(basis, perms, flips=None):
  """[n_ops][D][D]: (P_k v)(x) = v(row_k(x))."""
  basis = np.asarray(basis, np.float32)
  index = lookup(basis)
  perms = np.asarray(perms, np.int64).reshape(-1, basis.shape[1])
  flips = np.zeros(len(perms), np.int64) if flips is None else np.asarray(flips, np.int64).ravel()
  out = np.zeros((len(perms), len(basis), len(basis)))
  rows = np.arange(len(basis))
  for k, (perm, flip) in enumerate(zip(perms, flips)):
    out[k, rows, index(so.rows(basis, perm, flip))] = 1.0
  return out


def exact_sectors(vector, basis, hmat, perms, flips, chi):
  """(weight [n_sectors], energy [n_sectors], plain energy): the estimator's expectation values under |v|^2 by full
  enumeration -- weight_s = <v|P_s|v> / <v|v>, energy_s = <v|H P_s|v> / <v|P_s|v> (nan where the weight is exactly 0),
  P_s = sum_k chi[s][k] P_k."""
  v = np.asarray(vector, np.float64)
  ops = op_matrices(basis, perms, flips)
  chi = np.asarray(chi, np.float64).reshape(-1, len(ops))
  pv = np.einsum('sk,kxy,y->sx', chi, ops, v)                                  # (P_s v)(x)
  hv = hmat @ v
  norm = v @ v
  num, den = pv @ hv, pv @ v
  with np.errstate(divide='ignore', invalid='ignore'):
    energy = np.where(den != 0, num / den, np.nan)
  return den / norm, energy, float(v @ hv / norm)

"""fp64 restatement of the symmetrized ansatz for the tests: psi_s(x) = sum_k chi_k psi(g_k x).

An op k is a site permutation perm_k, optionally followed by the global spin flip: row_k(x)[i] = f_k x[perm_k[i]]
(the convention of lattice.translations and VmcEngine.symmetry_expectations).  The base is a tests.prod_oracle.Factor;
theta and the parameter count are the base's.  local_energy is the DIRECT vo.local_value of psi_s -- the sum over
connected configurations of psi_s itself --, never the fold sum_k c_k E_loc^psi(g_k x): the fold identity the library
rests on is what the tests check, so the oracle must not assume it (local_energy_fold states it, for that check).
prod_oracle.energy_gradient_accumulate and prod_oracle.mc_step work on this class unchanged.
"""
import numpy as np

from oracle import vmc_oracle as vo


class Symmetrized:

  def __init__(self, base, perms, flips=None, characters=None):
    self.base = base
    self.perms = np.asarray(perms, np.int64).reshape(-1, np.asarray(perms).shape[-1])
    self.n_ops = len(self.perms)
    self.flips = np.zeros(self.n_ops, np.int64) if flips is None else np.asarray(flips, np.int64).ravel()
    self.chi = np.ones(self.n_ops) if characters is None else np.asarray(characters, np.float64).ravel()
    assert self.flips.size == self.n_ops and self.chi.size == self.n_ops
    self.theta, self.num_params = base.theta, base.num_params

  def rows(self, configs):
    """[n_ops][B][N] float32: the permuted (and flipped) configurations."""
    c = np.asarray(configs, np.float32)
    sign = np.where(self.flips != 0, -1.0, 1.0).astype(np.float32)
    return sign[:, None, None] * c[:, self.perms].transpose(1, 0, 2)

  def terms(self, configs):
    """[n_ops][B] fp64: chi_k psi(g_k x)."""
    rows = self.rows(configs)
    n, b, sites = rows.shape
    psi = np.asarray(self.base.psi(rows.reshape(n * b, sites)), np.float64).reshape(n, b)
    return self.chi[:, None] * psi

  def psi(self, configs):
    return self.terms(configs).sum(0)

  def A(self, configs):
    return np.abs(self.terms(configs)).sum(0)

  def cancellation(self, configs):
    """r = |S| / A in [0, 1]: 1 without cancellation, 0 at a structural zero."""
    t = self.terms(configs)
    return np.abs(t.sum(0)) / np.abs(t).sum(0)

  def weights(self, configs):
    """c_k(x) = chi_k psi(g_k x) / psi_s(x), [n_ops][B]; they sum to one over k."""
    t = self.terms(configs)
    return t / t.sum(0)

  def log_grads(self, configs):
    """O^s [B][P] = sum_k chi_k psi_k O(g_k x) / psi_s."""
    rows = self.rows(configs)
    n, b, sites = rows.shape
    o = np.asarray(self.base.log_grads(rows.reshape(n * b, sites)), np.float64).reshape(n, b, -1)
    return np.einsum('kb,kbp->bp', self.weights(configs), o)

  def local_energy(self, configs, bonds, j_x, j_z):
    return vo.local_value(self.psi, np.asarray(configs, np.float32), bonds, j_x, j_z, dtype=np.float64)

  def local_energy_fold(self, configs, bonds, j_x, j_z):
    """sum_k c_k(x) E_loc^psi(g_k x): equal to local_energy when every op is a symmetry of the Hamiltonian."""
    rows = self.rows(configs)
    n, b, sites = rows.shape
    e = vo.local_value(lambda c: np.asarray(self.base.psi(c), np.float64), rows.reshape(n * b, sites), bonds, j_x, j_z,
                       dtype=np.float64).reshape(n, b)
    return (self.weights(configs) * e).sum(0)


def sector_hamiltonian_levels(n_sites, bonds, j_x, j_z, perms, flips, characters):
  """Eigenvalues (ascending) of the Heisenberg Hamiltonian inside the sector P = sum_k chi_k g_k of the Sz = 0 block, by
  dense diagonalisation: the block is built over the Sz = 0 configurations, P as a matrix over them, and the spectrum of H
  on the range of P is returned (P a projector: chi the characters of lattice.sector_characters)."""
  import itertools
  ups = list(itertools.combinations(range(n_sites), n_sites // 2))
  cfgs = -np.ones((len(ups), n_sites))
  for r, u in enumerate(ups):
    cfgs[r, list(u)] = 1.0
  index = {tuple(c): r for r, c in enumerate(cfgs)}
  dim = len(cfgs)
  jx = np.broadcast_to(np.asarray(j_x, np.float64), (len(bonds),))
  jz = np.broadcast_to(np.asarray(j_z, np.float64), (len(bonds),))
  h = np.zeros((dim, dim))
  for r, c in enumerate(cfgs):
    for (i, j), x, z in zip(bonds, jx, jz):
      h[r, r] += 0.25 * z * c[i] * c[j]
      if c[i] != c[j]:
        d = c.copy(); d[i], d[j] = c[j], c[i]
        h[index[tuple(d)], r] += 0.5 * x
  perms = np.asarray(perms, np.int64)
  flips = np.zeros(len(perms), np.int64) if flips is None else np.asarray(flips, np.int64)
  p = np.zeros((dim, dim))
  for g, f, chi in zip(perms, flips, np.asarray(characters, np.float64)):
    for r, c in enumerate(cfgs):
      p[index[tuple((-1.0 if f else 1.0) * c[g])], r] += chi      # |x> -> |g x>
  w, v = np.linalg.eigh((p + p.T) / 2)
  basis = v[:, w > 0.5]
  return np.linalg.eigvalsh(basis.T @ h @ basis)

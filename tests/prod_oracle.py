"""fp64 restatement of the product of two wavefunctions ('prod', wavefunctions.py:107-161) for the tests.

psi(x) = psi_a(x) psi_b(x); theta = a's parameters followed by b's; O_k of a factor is its own d ln|psi_f| / d theta_k.
The factors come from oracle.vmc_oracle (fully_connected, rbm), tests.pbdg_oracle and tests.edvec_oracle; the sampler,
the Hamiltonian and the accumulator formulas come from oracle.vmc_oracle through an amp_fn.
"""
import numpy as np

from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo
from tests import pbdg_oracle as po


class Factor:
  """psi(configs) -> fp64 amplitudes (shift applied); log_grads(configs) -> O [B, P]."""

  def __init__(self, kind, theta, psi, log_grads, shift=0.0):
    self.kind, self.theta, self.psi, self.log_grads, self.shift = kind, np.asarray(theta, np.float64), psi, log_grads, shift
    self.num_params = self.theta.size


def fc_factor(theta, layer_size, num_layers, shift=-10.0):
  psi = lambda c: vo.fc_psi(theta, c, layer_size, num_layers, shift, dtype=np.float64)
  grads = lambda c: vo.per_sample_logit_grads(theta, c, layer_size, num_layers, dtype=np.float64)
  return Factor('fully_connected', theta, psi, grads, shift)


def rbm_factor(theta, layer_size, num_layers, shift=-10.0):
  psi = lambda c: vo.rbm_psi(theta, c, layer_size, num_layers, shift, dtype=np.float64)
  grads = lambda c: vo.rbm_per_sample_logit_grads(theta, c, layer_size, num_layers, dtype=np.float64)
  return Factor('rbm', theta, psi, grads, shift)


def pbdg_factor(theta, shift=-10.0):
  return Factor('pbdg', theta, lambda c: po.psi(theta, c, shift), lambda c: po.log_derivatives(theta, c), shift)


def edvec_factor(vector, top, bot):
  vec = np.asarray(vector, np.float64)

  def grads(c):
    idx = eo.index(c, top, bot)
    o = np.zeros((len(idx), vec.size))
    p = vec[idx]
    keep = p != 0
    o[np.flatnonzero(keep), idx[keep]] = 1.0 / p[keep]
    return o
  return Factor('ed_vector', vec, lambda c: eo.amplitude(vec, c, top, bot), grads, 0.0)


class Product:
  def __init__(self, a, b):
    self.a, self.b = a, b
    self.num_params = a.num_params + b.num_params
    self.theta = np.concatenate([a.theta, b.theta])

  def psi(self, configs):
    c = np.asarray(configs, np.float32)
    return np.asarray(self.a.psi(c), np.float64) * np.asarray(self.b.psi(c), np.float64)

  def log_grads(self, configs):
    c = np.asarray(configs, np.float32)
    return np.concatenate([self.a.log_grads(c), self.b.log_grads(c)], axis=1)

  def local_energy(self, configs, bonds, j_x, j_z):
    return vo.local_value(self.psi, np.asarray(configs, np.float32), bonds, j_x, j_z, dtype=np.float64)


def energy_gradient_accumulate(acc, prod, configs, bonds, j_x, j_z):
  """training.py:539-558 on the product."""
  e_loc = prod.local_energy(configs, bonds, j_x, j_z)
  o = prod.log_grads(configs)
  acc.g1_total += o.sum(0); acc.g2_total += (e_loc[:, None] * o).sum(0); acc.g_count += 1
  acc.e_total += e_loc.sum(); acc.e_count += e_loc.size
  return e_loc


def log_overlap_accumulate(acc, prod, prod_omega, configs, bonds, j_x, j_z, beta):
  """training.py:661-695 on the product, signed amplitudes."""
  c = np.asarray(configs, np.float32)
  p, p_w = prod.psi(c), prod_omega.psi(c)
  h_psi_w = vo.apply_in_place(prod_omega.psi, c, bonds, j_x, j_z, p_w, np.float64)
  ratio = (p_w - beta * h_psi_w) / p
  e_loc = h_psi_w / p_w
  o = prod.log_grads(c)
  acc.g1_total += o.sum(0); acc.g2_total += (ratio[:, None] * o).sum(0); acc.g_count += 1
  acc.e_total += e_loc.sum(); acc.e_count += e_loc.size
  acc.r_total += ratio.sum(); acc.r_count += ratio.size
  return e_loc, ratio


def mc_step(prod, configs, i_up, i_dn, u):
  """graph_builders.py:67-88 with the product's amplitudes -> (new configs, accept mask, psi'/psi)."""
  c = np.asarray(configs, np.float32)
  new = c.copy()
  rows = np.arange(len(c))
  new[rows, i_up] = -1.0
  new[rows, i_dn] = 1.0
  p0, p1 = prod.psi(c), prod.psi(new)
  with np.errstate(divide='ignore', invalid='ignore'):
    ratio = p1 / p0
  acc = np.where(p0 == 0, p1 != 0, ratio ** 2 > np.asarray(u, np.float64))
  out = np.where(acc[:, None], new, c)
  return out, acc, ratio

"""numpy fp64 restatement of the ed_vector ansatz -- FullVector (wavefunctions.py:1001-1080): Lin tables of the Sz = 0
sector, index and amplitude, local energies, both accumulate modes and the exact energy of a vector.

Conventions: a configuration's up spins set bits, bot = sum_{i < N/2} [s_i > 0] 2^i, top the same over the upper half,
idx = top_table[top] + bot_table[bot], psi = vector[idx].  The tables built here enumerate the sector in ascending
(top, bot) order.  Test infrastructure; nothing here is used by the product path."""
import itertools

import numpy as np

from tests import exact_states


def popcounts(h):
  w = np.arange(1 << h)
  return sum((w >> i) & 1 for i in range(h))


def lin_tables(n):
  """(top_table, bot_table, length): top_table[t] = number of sector configurations whose upper half-word is below t,
  bot_table[b] = rank of b among the lower half-words of its popcount."""
  h = n // 2
  pop = popcounts(h)
  cls = np.array([np.sum(pop == k) for k in range(h + 1)], np.int64)       # C(h, k)
  top = np.concatenate([[0], np.cumsum(cls[h - pop])])[:-1]
  bot = np.zeros(1 << h, np.int64)
  for k in range(h + 1):
    bot[pop == k] = np.arange(cls[k])
  return top.astype(np.int32), bot.astype(np.int32), int(np.sum(cls[h - pop]))


def half_words(configs):
  cfg = np.asarray(configs)
  h = cfg.shape[1] // 2
  bits = (cfg > 0).astype(np.int64)
  weights = 1 << np.arange(h)
  return bits[:, h:] @ weights, bits[:, :h] @ weights              # (top, bot)


def index(configs, top_table, bot_table):
  t, b = half_words(configs)
  return np.asarray(top_table, np.int64)[t] + np.asarray(bot_table, np.int64)[b]


def amplitude(vector, configs, top_table, bot_table):
  return np.asarray(vector)[index(configs, top_table, bot_table)]


def sz0_configurations(n):
  """Every Sz = 0 configuration [C(n, n/2), n] of +-1, in the order of tests/exact_states.ed_ground_state."""
  combos = list(itertools.combinations(range(n), n // 2))
  cfg = np.ones((len(combos), n), np.float32)
  for k, c in enumerate(combos):
    cfg[k, list(c)] = -1
  return cfg


def vector_from_ed(n, bonds, jx, jz):
  """(E0, vector[len] in Lin order (fp64), top_table, bot_table)."""
  e0, vec, cfgs, _ = exact_states.ed_ground_state(n, bonds, jx, jz)
  top, bot, length = lin_tables(n)
  out = np.zeros(length)
  out[index(cfgs, top, bot)] = vec
  return float(e0), out, top, bot


def local_energy_terms(vector, configs, top_table, bot_table, bonds, j_x, j_z):
  """(diag [B], terms [B, n_bonds]): 1/4 jz s_i s_j summed, and 1/2 jx psi'/psi per antiparallel bond (0 elsewhere), fp64."""
  cfg = np.asarray(configs, np.float64)
  vec = np.asarray(vector, np.float64)
  nb = len(bonds)
  jx = np.broadcast_to(np.asarray(j_x, np.float64), (nb,))
  jz = np.broadcast_to(np.asarray(j_z, np.float64), (nb,))
  psi = vec[index(cfg, top_table, bot_table)]
  diag = np.zeros(len(cfg))
  terms = np.zeros((len(cfg), nb))
  for k, (i, j) in enumerate(bonds):
    sz = cfg[:, i] * cfg[:, j]
    diag += 0.25 * jz[k] * sz
    anti = sz < 0
    swapped = cfg[anti].copy()
    swapped[:, [i, j]] = swapped[:, [j, i]]
    with np.errstate(divide='ignore', invalid='ignore'):
      terms[anti, k] = 0.5 * jx[k] * vec[index(swapped, top_table, bot_table)] / psi[anti]
  return diag, terms


def local_energy(vector, configs, top_table, bot_table, bonds, j_x, j_z):
  diag, terms = local_energy_terms(vector, configs, top_table, bot_table, bonds, j_x, j_z)
  return diag + terms.sum(1)


def accumulate(vector, configs, top_table, bot_table, weights):
  """g1[k] = sum_b delta(k, idx_b) / psi_b, g2[k] = sum_b w_b delta(k, idx_b) / psi_b (chains with psi_b = 0 add
  nothing), the sums of |terms| per entry and the number of chains per entry: (g1, g2, a1, a2, count), fp64."""
  vec = np.asarray(vector, np.float64)
  idx = index(configs, top_table, bot_table)
  psi = vec[idx]
  w = np.asarray(weights, np.float64)
  keep = psi != 0
  out = [np.zeros(len(vec)) for _ in range(5)]
  np.add.at(out[0], idx[keep], 1.0 / psi[keep])
  np.add.at(out[1], idx[keep], w[keep] / psi[keep])
  np.add.at(out[2], idx[keep], np.abs(1.0 / psi[keep]))
  np.add.at(out[3], idx[keep], np.abs(w[keep] / psi[keep]))
  np.add.at(out[4], idx[keep], 1.0)
  return tuple(out)


def itswo_ratio_fp32(psi, psi_omega, eloc_omega, beta):
  """(psi_w / psi) (1 - beta E_w) in fp32, one IEEE operation per step (training.py:665-672): the weights of the
  LogOverlapITSWO accumulators as the fp32 pipeline forms them."""
  f = np.float32
  with np.errstate(divide='ignore', invalid='ignore'):
    return (np.asarray(psi_omega, f) / np.asarray(psi, f)) * (f(1.0) - f(beta) * np.asarray(eloc_omega, f))


def exact_energy(vector, n, top_table, bot_table, bonds, j_x, j_z):
  """<v|H|v> / <v|v> over the whole sector."""
  cfg = sz0_configurations(n)
  vec = np.asarray(vector, np.float64)
  psi = vec[index(cfg, top_table, bot_table)]
  nz = psi != 0
  e = np.zeros(len(cfg))
  e[nz] = local_energy(vec, cfg[nz], top_table, bot_table, bonds, j_x, j_z)
  return float(np.sum(psi[nz] ** 2 * e[nz]) / np.sum(psi ** 2))

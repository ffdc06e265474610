"""fp64 oracle of the Lanczos-step energies (vmc_energy_moments): the local values e = (H psi)(x) / psi(x) and
g = (H^2 psi)(x) / psi(x) of  H = sum_b j_x[b] (S+S- + S-S+) / 2 + j_z[b] SzSz,  restated independently of csrc/moments.hip.

local_values applies H twice to the basis vector of a chain, as a dictionary {configuration: coefficient}: every ordered
pair of bonds is walked, nothing is shared between (a, b) and (b, a), and nothing is skipped for a == b.  H is real and
symmetric, so (H^n psi)(x) = sum_y (H^n e_x)(y) psi(y).  The couplings enter as the engine holds them: hx = fp32(j_x) / 2 and
qz = fp32(j_z) / 4, both exact.

n_rows2 and second_order_rows restate the three rules of the compacted list; dense_h builds H over the Sz = 0 basis for the
CPU identities."""
import itertools

import numpy as np


def couplings(n_bonds, j_x, j_z):
  """(hx, qz) fp64 [n_bonds] from scalars or per-bond arrays, rounded to fp32 first as vmc_set_bonds takes them."""
  jx = np.broadcast_to(np.asarray(j_x, np.float32), (n_bonds,)).astype(np.float64)
  jz = np.broadcast_to(np.asarray(j_z, np.float32), (n_bonds,)).astype(np.float64)
  return 0.5 * jx, 0.25 * jz


def apply_h(state, bonds, hx, qz):
  """H applied to {configuration tuple: coefficient}."""
  out = {}
  for y, v in state.items():
    d = 0.0
    for b, (i, j) in enumerate(bonds):
      d += qz[b] * y[i] * y[j]
      if y[i] != y[j]:
        z = list(y)
        z[i], z[j] = z[j], z[i]
        z = tuple(z)
        out[z] = out.get(z, 0.0) + hx[b] * v
    out[y] = out.get(y, 0.0) + d * v
  return out


def local_values(psi, cfg, bonds, j_x, j_z):
  """(e [B], g [B], alive [B] bool) in fp64; e = g = 0 where the chain's own amplitude vanishes.  psi(configs [M][N]) -> [M]."""
  cfg = np.asarray(cfg, np.float32)
  hx, qz = couplings(len(bonds), j_x, j_z)
  rows1, rows2 = [], []
  for x in cfg:
    r1 = apply_h({tuple(float(s) for s in x): 1.0}, bonds, hx, qz)
    rows1.append(r1)
    rows2.append(apply_h(r1, bonds, hx, qz))
  every = sorted(set().union(*[set(r) for r in rows2], *[set(r) for r in rows1]))
  amp = dict(zip(every, np.asarray(psi(np.array(every, np.float32)), np.float64)))
  own = np.asarray(psi(cfg), np.float64)
  e, g = np.zeros(len(cfg)), np.zeros(len(cfg))
  for c in range(len(cfg)):
    if own[c] == 0:
      continue
    e[c] = sum(v * amp[y] for y, v in sorted(rows1[c].items())) / own[c]
    g[c] = sum(v * amp[y] for y, v in sorted(rows2[c].items())) / own[c]
  return e, g, own != 0


def _swapped(x, bond):
  y = list(x)
  y[bond[0]], y[bond[1]] = y[bond[1]], y[bond[0]]
  return tuple(y)


def second_order_rows(x, bonds):
  """The compacted list of one chain by the three rules: (first [(a, x^a)], rows [(a, b, multiplicity, x^{ab})],
  selfs [(a, b)]): `first` the antiparallel bonds ascending; per a the bonds b antiparallel on x^a ascending -- b on the site
  pair of a: no row (selfs); b disjoint from a: one row for a < b, multiplicity 2; b sharing one site: one row."""
  x = tuple(float(s) for s in x)
  first, rows, selfs = [], [], []
  for a, ba in enumerate(bonds):
    if x[ba[0]] == x[ba[1]]:
      continue
    xa = _swapped(x, ba)
    first.append((a, xa))
    for b, bb in enumerate(bonds):
      if xa[bb[0]] == xa[bb[1]]:
        continue
      common = len(set(ba) & set(bb))
      if common == 2:
        selfs.append((a, b))
      elif common == 0:
        if a < b:
          rows.append((a, b, 2.0, _swapped(xa, bb)))
      else:
        rows.append((a, b, 1.0, _swapped(xa, bb)))
  return first, rows, selfs


def n_rows2(cfg, bonds):
  return sum(len(second_order_rows(x, bonds)[1]) for x in np.asarray(cfg))


def sz0_basis(n):
  """Every Sz = 0 configuration [C(n, n / 2)][n] of +-1 and {tuple: index}."""
  combos = list(itertools.combinations(range(n), n // 2))
  cfg = np.ones((len(combos), n), np.float32)
  for k, c in enumerate(combos):
    cfg[k, list(c)] = -1
  return cfg, {tuple(float(s) for s in row): k for k, row in enumerate(cfg)}


def dense_h(n, bonds, j_x, j_z):
  """(basis [D][n], H [D][D] fp64) over the Sz = 0 basis, element by element from the definition."""
  hx, qz = couplings(len(bonds), j_x, j_z)
  cfg, index = sz0_basis(n)
  h = np.zeros((len(cfg), len(cfg)))
  for k, row in enumerate(cfg):
    for b, (i, j) in enumerate(bonds):
      h[k, k] += qz[b] * row[i] * row[j]
      if row[i] != row[j]:
        other = row.copy()
        other[i], other[j] = row[j], row[i]
        h[index[tuple(float(s) for s in other)], k] += hx[b]
  return cfg, h


def exact_moments(h, vec):
  """h1 .. h4 = <v| H^n |v> / <v|v> and the exact Lanczos step from them: (h [4], E1, alpha, var1)."""
  v = np.asarray(vec, np.float64)
  hv = h @ v
  hhv = h @ hv
  norm = v @ v
  hn = np.array([v @ hv, hv @ hv, hv @ hhv, hhv @ hhv]) / norm
  a = np.array([[hn[0], hn[1]], [hn[1], hn[2]]])
  s = np.array([[1.0, hn[0]], [hn[0], hn[1]]])
  w, vecs = np.linalg.eig(np.linalg.solve(s, a))
  k = int(np.argmin(w.real))
  alpha = float((vecs[1, k] / vecs[0, k]).real)
  e1 = float(w[k].real)
  var1 = (hn[1] + 2 * alpha * hn[2] + alpha * alpha * hn[3]) / (1 + 2 * alpha * hn[0] + alpha * alpha * hn[1]) - e1 * e1
  return hn, e1, alpha, float(var1)

"""Bond-list helpers (the reference only has the inline 1-D default of
run_training.py:109 and the J.txt reader of run_training.py:103-107)."""
import os

import numpy as np


def chain_bonds(n_sites):
  """run_training.py:109: 1-D periodic chain."""
  return [(i, (i + 1) % n_sites) for i in range(0, n_sites)]


def torus_bonds(size_x, size_y, next_nearest=False):
  """size_x x size_y periodic square lattice, site = x + size_x*y, each bond once."""
  bonds = []
  for y in range(size_y):
    for x in range(size_x):
      s = x + size_x * y
      bonds.append((s, (x + 1) % size_x + size_x * y))
      bonds.append((s, x + size_x * ((y + 1) % size_y)))
  if next_nearest:
    for y in range(size_y):
      for x in range(size_x):
        s = x + size_x * y
        bonds.append((s, (x + 1) % size_x + size_x * ((y + 1) % size_y)))
        bonds.append((s, (x - 1) % size_x + size_x * ((y + 1) % size_y)))
  return bonds


def chain_coords(n_sites):
  """Positions [n_sites][1] of the sites of chain_bonds."""
  return np.arange(n_sites, dtype=np.float64).reshape(n_sites, 1)


def torus_coords(size_x, size_y):
  """Positions [size_x * size_y][2] of the sites of torus_bonds: site = x + size_x * y sits at (x, y)."""
  s = np.arange(size_x * size_y)
  return np.stack([s % size_x, s // size_x], axis=1).astype(np.float64)


def chain_momenta(n_sites):
  """The momenta a periodic chain allows: q = 2 pi m / n_sites, m = 0 .. n_sites - 1; [n_sites][1]."""
  return (2.0 * np.pi * np.arange(n_sites) / n_sites).reshape(n_sites, 1)


def torus_momenta(size_x, size_y):
  """The momenta the size_x x size_y torus allows, (2 pi m_x / size_x, 2 pi m_y / size_y), m_x fastest; [N][2]."""
  m = np.arange(size_x * size_y)
  return np.stack([2.0 * np.pi * (m % size_x) / size_x, 2.0 * np.pi * (m // size_x) / size_y], axis=1)


def all_pairs(n):
  """Every pair (i, j), i < j, of n sites: [n (n - 1) / 2][2] int32, i-major."""
  i, j = np.triu_indices(n, k=1)
  return np.stack([i, j], axis=1).astype(np.int32)


def structure_factor(ss, pairs, coords, qs):
  """S(q) = (1 / N) [3 N / 4 + 2 sum_{i<j} cos(q . (r_i - r_j)) <S_i . S_j>] for every q of `qs` [n_q][d], from
  ss [n_pairs] = <S_i . S_j> of `pairs` [n_pairs][2] (every pair of distinct sites once, in either order; a pair that
  is missing counts as uncorrelated) and the positions coords [N][d].  3 N / 4 is the i = j part, S (S + 1) per site."""
  ss = np.asarray(ss, np.float64).ravel()
  pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
  coords = np.asarray(coords, np.float64)
  coords = coords.reshape(coords.shape[0], -1)
  qs = np.asarray(qs, np.float64).reshape(-1, coords.shape[1])
  if ss.size != pairs.shape[0]:
    raise ValueError('structure_factor: {} values for {} pairs'.format(ss.size, pairs.shape[0]))
  n = coords.shape[0]
  dr = coords[pairs[:, 0]] - coords[pairs[:, 1]]          # [n_pairs][d]
  return (0.75 * n + 2.0 * np.cos(qs @ dr.T) @ ss) / n


def block_regions(num_sites, max_len=None):
  """The contiguous blocks [0, l), l = 1 .. max_len (default num_sites // 2), as a list of site lists: the regions
  whose second Renyi entropy a chain's (or a row-major cluster's) entanglement scaling is read from."""
  max_len = num_sites // 2 if max_len is None else int(max_len)
  if max_len < 0 or max_len > num_sites:
    raise ValueError('block_regions: max_len {} outside 0 .. {}'.format(max_len, num_sites))
  return [list(range(l)) for l in range(1, max_len + 1)]


def read_regions(path):
  """Regions from a text file: one region per line as site indices separated by blanks or commas; `#` starts a
  comment, a line without any index is skipped (the empty region cannot be written: pass it as [])."""
  regions = []
  with open(path) as f:
    for number, line in enumerate(f, 1):
      fields = line.split('#', 1)[0].replace(',', ' ').split()
      if not fields:
        continue
      try:
        regions.append([int(x) for x in fields])
      except ValueError:
        raise ValueError('{}:{}: a region is a line of integer site indices, got {!r}'.format(path, number, line.strip()))
  return regions


def region_masks(regions, num_sites):
  """[n_regions][num_sites] uint8 0/1 masks of `regions`: a two-dimensional array of zeros and ones (or booleans) with
  num_sites columns is taken as the masks themselves, anything else as a list of site lists (a site out of range or
  named twice: ValueError)."""
  if isinstance(regions, np.ndarray) and regions.ndim == 2 and regions.shape[1] == num_sites \
      and (regions.dtype == np.bool_ or (np.issubdtype(regions.dtype, np.number) and np.isin(regions, (0, 1)).all())):
    return np.ascontiguousarray(regions.astype(np.uint8))
  if isinstance(regions, np.ndarray) and regions.dtype == np.bool_:
    raise ValueError('region masks must have shape [n_regions][{}], got {}'.format(num_sites, regions.shape))
  regions = list(regions)
  masks = np.zeros((len(regions), num_sites), np.uint8)
  for k, region in enumerate(regions):
    sites = np.asarray(region)
    if sites.size and not np.issubdtype(sites.dtype, np.integer):
      raise ValueError('region {}: site indices must be integers'.format(k))
    sites = sites.astype(np.int64).ravel()
    if sites.size and (sites.min() < 0 or sites.max() >= num_sites):
      raise ValueError('region {}: site index out of range 0 .. {}'.format(k, num_sites - 1))
    if np.unique(sites).size != sites.size:
      raise ValueError('region {}: a site is named twice (a 0/1 mask must have {} columns)'.format(k, num_sites))
    masks[k, sites] = 1
  return masks


def all_bond_pairs(n_bonds):
  """Every ordered pair (a, b) of n_bonds bonds, a == b included: [n_bonds^2][2] int32, a-major."""
  a, b = np.divmod(np.arange(n_bonds * n_bonds), max(n_bonds, 1))
  return np.ascontiguousarray(np.stack([a, b], axis=1).astype(np.int32))


def read_bond_pairs(path):
  """(bonds, pairs) from a text file for the dimer-dimer correlations: a line `i j` names a bond, a line `i j k l` the
  pair of the bonds (i, j) and (k, l); blanks or commas separate, `#` starts a comment, a line without any index is
  skipped.  bonds: the distinct (i, j), as written, in the order of their first appearance; pairs: (a, b) indices into
  bonds, one per four-index line, in the file's order (empty when the file names bonds only)."""
  bonds, index, pairs = [], {}, []

  def bond(i, j):
    if (i, j) not in index:
      index[(i, j)] = len(bonds)
      bonds.append([i, j])
    return index[(i, j)]
  with open(path) as f:
    for number, line in enumerate(f, 1):
      fields = line.split('#', 1)[0].replace(',', ' ').split()
      if not fields:
        continue
      try:
        sites = [int(x) for x in fields]
      except ValueError:
        sites = []
      if len(sites) not in (2, 4):
        raise ValueError('{}:{}: a line is a bond `i j` or a pair of bonds `i j k l` of integer site indices, got {!r}'
                         .format(path, number, line.strip()))
      a = bond(sites[0], sites[1])
      if len(sites) == 4:
        pairs.append([a, bond(sites[2], sites[3])])
  return bonds, pairs


def bond_orientations(bonds, size_x, size_y=1):
  """(axis [n_bonds], origin [n_bonds]) of `bonds` on the size_x x size_y torus of torus_bonds (site = x + size_x * y;
  size_y = 1: the periodic chain): axis 0 / 1 for a nearest-neighbour bond along x / y with `origin` the site it leaves
  in the positive direction, axis -1 (origin -1) for any other pair of sites."""
  bonds = np.asarray(bonds, np.int64).reshape(-1, 2)
  axis = np.full(len(bonds), -1, np.int64)
  origin = np.full(len(bonds), -1, np.int64)
  for n, (i, j) in enumerate(bonds.tolist()):
    for s, t in ((i, j), (j, i)):
      xs, ys, xt, yt = s % size_x, s // size_x, t % size_x, t // size_x
      if axis[n] < 0 and ys == yt and xt == (xs + 1) % size_x and size_x > 1:
        axis[n], origin[n] = 0, s
      if axis[n] < 0 and xs == xt and yt == (ys + 1) % size_y and size_y > 1:
        axis[n], origin[n] = 1, s
  return axis, origin


def dimer_structure_factor(bonds, pairs, connected, size_x, size_y=1, qs=None):
  """Dimer structure factors of the nearest-neighbour bonds of the size_x x size_y torus (size_y = 1: the periodic
  chain) from connected [n_pairs] = <A B> - <A><B> of the bond pairs `pairs` [n_pairs][2] (indices into `bonds`):
    D_alpha(q) = (1 / n_alpha) sum over the pairs (a, b) of two alpha-oriented bonds of cos(q . (r_a - r_b)) connected(a, b)
  with r_a the site bond a leaves in the positive direction (bond_orientations) and n_alpha the number of distinct
  first bonds a among those pairs: all ordered pairs give the usual (1 / N_bonds) sum_{a, b}, one reference bond
  against all gives sum_b cos(q . (r_b - r_0)) connected(0, b) -- the same number on a translation-invariant state.
  Pairs of differently oriented bonds and pairs with a bond that is no nearest-neighbour bond do not enter.  Returns
  (qs [n_q][d], D [d][n_q]) with d = 1 (chain) or 2, row 0 the x-oriented and row 1 the y-oriented bonds, at the momenta
  the cluster allows (chain_momenta / torus_momenta) unless `qs` gives others."""
  bonds = np.asarray(bonds, np.int64).reshape(-1, 2)
  pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
  connected = np.asarray(connected, np.float64).ravel()
  if connected.size != pairs.shape[0]:
    raise ValueError('dimer_structure_factor: {} values for {} pairs'.format(connected.size, pairs.shape[0]))
  if pairs.size and (pairs.min() < 0 or pairs.max() >= len(bonds)):
    raise ValueError('dimer_structure_factor: a pair names a bond outside 0 .. {}'.format(len(bonds) - 1))
  if size_x < 1 or size_y < 1:
    raise ValueError('dimer_structure_factor: lattice sizes must be positive')
  chain = size_y == 1
  coords = chain_coords(size_x) if chain else torus_coords(size_x, size_y)
  if qs is None:
    qs = chain_momenta(size_x) if chain else torus_momenta(size_x, size_y)
  qs = np.asarray(qs, np.float64).reshape(-1, coords.shape[1])
  if bonds.size and (bonds.min() < 0 or bonds.max() >= len(coords)):
    raise ValueError('dimer_structure_factor: a bond names a site outside the {} x {} lattice'.format(size_x, size_y))
  axis, origin = bond_orientations(bonds, size_x, size_y)
  out = np.zeros((coords.shape[1], len(qs)))
  for alpha in range(coords.shape[1]):
    use = (axis[pairs[:, 0]] == alpha) & (axis[pairs[:, 1]] == alpha)
    if not use.any():
      continue
    a, b = pairs[use, 0], pairs[use, 1]
    dr = coords[origin[a]] - coords[origin[b]]              # [n_used][d]
    out[alpha] = np.cos(qs @ dr.T) @ connected[use] / np.unique(a).size
  return qs, out


def translations(size_x, size_y=1):
  """The N = size_x * size_y translations of the size_x x size_y torus of torus_bonds (site = x + size_x * y; size_y = 1:
  the periodic chain) as site permutations, [N][N] int32: op r = r_x + size_x * r_y has
  perm[x + size_x * y] = (x + r_x) mod size_x + size_x * ((y + r_y) mod size_y), so that the row of a configuration s is
  row[i] = s[perm[i]] (VmcEngine.symmetry_expectations).  Op 0 is the identity."""
  if size_x < 1 or size_y < 1:
    raise ValueError('translations: lattice sizes must be positive')
  s = np.arange(size_x * size_y)
  x, y = s % size_x, s // size_x
  r_x, r_y = x[:, None], y[:, None]
  return np.ascontiguousarray(((x[None, :] + r_x) % size_x + size_x * ((y[None, :] + r_y) % size_y)).astype(np.int32))


def point_group(size_x, size_y=1):
  """(labels, perms [n][N] int32) of the point group about site 0 of the size_x x size_y torus (site = x + size_x * y), as
  site permutations in the convention of `translations`: the periodic chain (size_y = 1) has the identity and the mirror
  x -> -x; a rectangle the identity, mirror_x (x -> -x), mirror_y (y -> -y) and the inversion; a square the eight elements of
  C4v: identity, rot90 ((x, y) -> (-y, x)), rot180, rot270, mirror_x, mirror_y, mirror_diag ((x, y) -> (y, x)) and
  mirror_antidiag ((x, y) -> (-y, -x)).  The identity comes first."""
  if size_x < 1 or size_y < 1:
    raise ValueError('point_group: lattice sizes must be positive')
  s = np.arange(size_x * size_y)
  x, y = s % size_x, s // size_x
  site = lambda u, v: ((u % size_x) + size_x * (v % size_y)).astype(np.int32)
  if size_y == 1:
    ops = [('identity', site(x, y)), ('mirror', site(-x, y))]
  elif size_x != size_y:
    ops = [('identity', site(x, y)), ('mirror_x', site(-x, y)), ('mirror_y', site(x, -y)), ('inversion', site(-x, -y))]
  else:
    ops = [('identity', site(x, y)), ('rot90', site(-y, x)), ('rot180', site(-x, -y)), ('rot270', site(y, -x)),
           ('mirror_x', site(-x, y)), ('mirror_y', site(x, -y)), ('mirror_diag', site(y, x)),
           ('mirror_antidiag', site(-y, -x))]
  return [name for name, _ in ops], np.ascontiguousarray(np.stack([p for _, p in ops]))


def check_symmetry_ops(perms, flips, num_sites):
  """(perms int32 [n_ops][num_sites], flips uint8 [n_ops]), contiguous, of the ops of VmcEngine.symmetry_expectations:
  every row of `perms` must be a permutation of 0 .. num_sites - 1 (one row alone is taken as one op), `flips` one 0 / 1
  (or boolean) per op, None: no flips.  Anything else is a ValueError that names the op: the rows of pbdg,
  fully_connected_nnb and ed_vector must stay at Sz = 0, which a bijection and a global flip keep and nothing else need."""
  p = np.asarray(perms)
  if p.ndim == 1 and p.size:
    p = p.reshape(1, -1)
  if p.ndim != 2 or p.shape[0] < 1:
    raise ValueError('symmetry ops: at least one site permutation of shape [{}] required'.format(num_sites))
  if not (np.issubdtype(p.dtype, np.integer) or (np.issubdtype(p.dtype, np.floating) and (p == np.rint(p)).all())):
    raise ValueError('symmetry ops: site indices must be integers')
  if p.shape[1] != num_sites:
    raise ValueError('symmetry ops: op 0 has {} entries, {} sites required'.format(p.shape[1], num_sites))
  p = p.astype(np.int64)
  for k, g in enumerate(p):
    if g.min() < 0 or g.max() >= num_sites:
      i = int(np.flatnonzero((g < 0) | (g >= num_sites))[0])
      raise ValueError('symmetry ops: op {}: entry {} = {} is no site in 0 .. {}'.format(k, i, int(g[i]), num_sites - 1))
    if np.unique(g).size != num_sites:
      raise ValueError('symmetry ops: op {}: a site is named twice (a permutation of 0 .. {} required)'.format(k, num_sites - 1))
  if flips is None:
    f = np.zeros(p.shape[0], np.int64)
  else:
    f = np.asarray(flips)
    if f.dtype != np.bool_ and not np.issubdtype(f.dtype, np.integer):
      raise ValueError('symmetry ops: flips are 0 or 1')
    f = f.astype(np.int64).ravel()
    if f.size != p.shape[0]:
      raise ValueError('symmetry ops: {} flips for {} ops'.format(f.size, p.shape[0]))
    bad = np.flatnonzero((f < 0) | (f > 1))
    if bad.size:
      raise ValueError('symmetry ops: op {}: flip = {}, 0 or 1 required'.format(int(bad[0]), int(f[bad[0]])))
  return np.ascontiguousarray(p.astype(np.int32)), np.ascontiguousarray(f.astype(np.uint8))


def read_symmetry_ops(path):
  """(perms, flips) from a text file: one op per line, an optional leading word `flip` (the global spin flip follows the
  permutation), then the site indices perm[0] perm[1] ... separated by blanks or commas; `#` starts a comment, a line
  without any field is skipped.  Lists, in the file's order; check_symmetry_ops validates them."""
  perms, flips = [], []
  with open(path) as f:
    for number, line in enumerate(f, 1):
      fields = line.split('#', 1)[0].replace(',', ' ').split()
      if not fields:
        continue
      flip = fields[0].lower() == 'flip'
      try:
        perm = [int(x) for x in fields[1 if flip else 0:]]
      except ValueError:
        perm = []
      if not perm:
        raise ValueError('{}:{}: an op is a line of integer site indices, optionally after the word `flip`, got {!r}'
                         .format(path, number, line.strip()))
      perms.append(perm)
      flips.append(int(flip))
  return perms, flips


def write_symmetry_ops(path, perms, flips=None, labels=None):
  """Writes what read_symmetry_ops reads; `labels` go into a trailing comment per line."""
  with open(path, 'w') as f:
    for k, perm in enumerate(perms):
      f.write('{}{}{}\n'.format('flip ' if flips is not None and flips[k] else '', ' '.join(str(int(i)) for i in perm),
                                '' if labels is None else '   # {}'.format(labels[k])))


def momentum_weights(values, size_x, size_y=1):
  """w[m] = (1 / N) sum_r cos(q_m . r) values[r] over the N = size_x * size_y values <T_r> of `translations` (the last axis
  of `values`; leading axes -- samples -- are kept), at the momenta q_m of torus_momenta (size_y = 1: chain_momenta), in
  their order.  For a real psi <T_r> = <T_-r>, so the cosine transform is the weight of the state at each momentum; the
  weights of q and -q are equal and each carries its own share; the weights sum to values[0]."""
  values = np.asarray(values, np.float64)
  n = size_x * size_y
  if size_x < 1 or size_y < 1 or values.ndim < 1 or values.shape[-1] != n:
    raise ValueError('momentum_weights: {} values for the {} x {} lattice'.format(values.shape[-1] if values.ndim else 0,
                                                                                   size_x, size_y))
  chain = size_y == 1
  coords = chain_coords(size_x) if chain else torus_coords(size_x, size_y)
  qs = chain_momenta(size_x) if chain else torus_momenta(size_x, size_y)
  return values @ np.cos(coords @ qs.T) / n


def sector_characters(size_x, size_y=1, spin_flip=False):
  """(labels, chi [n_sectors][n_ops] float64): the real characters of the symmetry sectors of the size_x x size_y torus
  (size_y = 1: the periodic chain) for the ops `translations(size_x, size_y)` -- with spin_flip followed by the same N
  translations after the global flip (n_ops = 2 N) -- as VmcEngine.projected_energy takes them.  One row per momentum
  class {k, -k} (psi is real: the two are not told apart), with spin_flip one per class and parity +-:
    chi[s][r, f] = mult cos(k . r) (+-1)^f / |G|,   mult = 2 unless k = -k,   |G| = n_ops
  so that P_s = sum_k chi[s][k] g_k are idempotent, mutually orthogonal projectors that sum to the identity: the rows of
  chi sum to the indicator of op 0.  Labels: `q<m>` on a chain, `q<m_x>,<m_y>` on a torus (k = 2 pi m / size, the class
  named by the smaller of the two momenta in torus_momenta's order), then `+` / `-` with spin_flip."""
  if size_x < 1 or size_y < 1:
    raise ValueError('sector_characters: lattice sizes must be positive')
  n = size_x * size_y
  r = np.arange(n)
  r_x, r_y = r % size_x, r // size_x
  labels, rows = [], []
  for m in range(n):
    m_x, m_y = m % size_x, m // size_x
    minus = (-m_x) % size_x + size_x * ((-m_y) % size_y)
    if minus < m:
      continue
    phase = (m_x * r_x * size_y + m_y * r_y * size_x) % n           # k . r = 2 pi phase / n, reduced exactly
    row = (1.0 if minus == m else 2.0) * np.cos(2.0 * np.pi * phase / n)
    name = 'q{}'.format(m_x) if size_y == 1 else 'q{},{}'.format(m_x, m_y)
    if not spin_flip:
      labels.append(name); rows.append(row / n)
    else:
      for sign, parity in ((1.0, '+'), (-1.0, '-')):
        labels.append(name + parity); rows.append(np.concatenate([row, sign * row]) / (2 * n))
  return labels, np.ascontiguousarray(np.stack(rows))


def write_characters(path, labels, chi):
  """A text table of characters: one row per sector, the label (no blanks) first, then chi[s][0] chi[s][1] ... with 17
  significant digits; `#` starts a comment."""
  chi = np.asarray(chi, np.float64)
  if chi.ndim != 2 or len(labels) != chi.shape[0] or any((not str(l)) or len(str(l).split()) != 1 or '#' in str(l) for l in labels):
    raise ValueError('write_characters: one label without blanks per row of a [n_sectors][n_ops] table required')
  with open(path, 'w') as f:
    f.write('# label chi[0] chi[1] ...\n')
    for label, row in zip(labels, chi):
      f.write('{} {}\n'.format(label, ' '.join(repr(float(x)) for x in row)))


def read_characters(path):
  """(labels, chi [n_sectors][n_ops] float64) of the table write_characters writes; every row needs the same number of
  finite characters."""
  labels, rows = [], []
  with open(path) as f:
    for number, line in enumerate(f, 1):
      fields = line.split('#', 1)[0].split()               # (blanks only: a torus label holds a comma)
      if not fields:
        continue
      try:
        row = [float(x) for x in fields[1:]]
      except ValueError:
        row = []
      if not row or not np.isfinite(row).all() or (rows and len(row) != len(rows[0])):
        raise ValueError('{}:{}: a sector is a label followed by one finite character per op, got {!r}'.format(
            path, number, line.strip()))
      labels.append(fields[0]); rows.append(row)
  if not rows:
    raise ValueError('{}: no sector'.format(path))
  return labels, np.asarray(rows, np.float64)


def check_characters(characters, n_ops):
  """chi float64 [n_sectors][n_ops], contiguous, of the characters of VmcEngine.projected_energy (one row alone is one
  sector); anything else, a non-finite character included, is a ValueError."""
  try:
    chi = np.asarray(characters, np.float64)
  except (TypeError, ValueError):
    raise ValueError('characters: a [n_sectors][{}] table of real numbers required'.format(n_ops))
  if chi.ndim == 1 and chi.size:
    chi = chi.reshape(1, -1)
  if chi.ndim != 2 or chi.shape[0] < 1:
    raise ValueError('characters: at least one sector of shape [{}] required'.format(n_ops))
  if chi.shape[1] != n_ops:
    raise ValueError('characters: {} characters per sector for {} ops'.format(chi.shape[1], n_ops))
  if not np.isfinite(chi).all():
    s, k = np.argwhere(~np.isfinite(chi))[0]
    raise ValueError('characters: sector {}: the character of op {} is not finite'.format(int(s), int(k)))
  return np.ascontiguousarray(chi)


def check_hamiltonian_symmetry(bonds, j_x, j_z, perms):
  """None when every site permutation of `perms` [n_ops][N] maps the Hamiltonian's bonds onto themselves -- the multiset
  of (unordered pair, float32 j_x, float32 j_z) over `bonds` is unchanged (a multiset: the 2-wide torus of torus_bonds
  names a bond twice); j_x / j_z: one value or one per bond -- else a ValueError that names the op and the first bond
  whose image is missing.  The mirror of plan_symm_check_hamiltonian (the library checks by itself); invariance under a
  permutation and under its inverse are the same statement; the global spin flip is always a symmetry of XXZ bonds."""
  from collections import Counter
  ij = np.asarray(bonds, np.int64).reshape(-1, 2)
  nb = len(ij)
  if nb < 1:
    raise ValueError('check_hamiltonian_symmetry: at least one bond required')
  bits = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (nb,))).view(np.uint32)   # one or one per bond
  jx, jz = bits(j_x), bits(j_z)
  perms = np.asarray(perms, np.int64)
  if perms.ndim == 1:
    perms = perms.reshape(1, -1)
  key = lambda a, b, x, z: (int(min(a, b)), int(max(a, b)), int(x), int(z))
  base = Counter(key(i, j, x, z) for (i, j), x, z in zip(ij, jx, jz))
  for k, g in enumerate(perms):
    left = base.copy()
    for b, ((i, j), x, z) in enumerate(zip(ij, jx, jz)):
      image = key(g[i], g[j], x, z)
      if left[image] < 1:
        raise ValueError('op {} is no symmetry of the Hamiltonian: bond {} = ({}, {}) goes to ({}, {}), which is no bond '
                         'with its couplings'.format(k, b, int(i), int(j), int(g[i]), int(g[j])))
      left[image] -= 1


def load_bonds(checkpoint_dir, n_sites):
  """run_training.py:103-109 / run_energy_evaluation.py:51-57: `J.txt` of integer pairs
  (extra columns ignored), else the periodic chain."""
  path = os.path.join(checkpoint_dir, 'J.txt')
  if os.path.exists(path):
    data = np.atleast_2d(np.genfromtxt(path, dtype=int))
    return [[int(bond[0]), int(bond[1])] for bond in data]
  return chain_bonds(n_sites)


def write_bonds(checkpoint_dir, bonds):
  with open(os.path.join(checkpoint_dir, 'J.txt'), 'w') as f:
    for i, j in bonds:
      f.write('{} {}\n'.format(i, j))


def jq_chain_terms(n_sites):
  """The four-spin terms of the periodic J-Q chain (operators.JQHamiltonian): (i, i + 1, i + 2, i + 3) for every i, the
  singlet projectors on the bonds (i, i + 1) and (i + 2, i + 3); [n_sites][4] int32.  n_sites >= 4."""
  if n_sites < 4:
    raise ValueError('jq_chain_terms: a term names four distinct sites, n_sites >= 4 required, got {}'.format(n_sites))
  i = np.arange(n_sites).reshape(n_sites, 1)
  return np.ascontiguousarray(((i + np.arange(4).reshape(1, 4)) % n_sites).astype(np.int32))


def jq_torus_terms(size_x, size_y):
  """The four-spin terms of the J-Q model on the size_x x size_y torus (site numbering of torus_coords): per plaquette
  with lower left corner s = (x, y) the two parallel horizontal bonds, (s, s + x^, s + y^, s + x^ + y^), then the two
  parallel vertical ones, (s, s + y^, s + x^, s + x^ + y^); [2 N][4] int32.  Both sizes >= 3."""
  if size_x < 3 or size_y < 3:
    raise ValueError('jq_torus_terms: both sizes >= 3 required (a smaller torus folds a plaquette onto itself), got '
                     '{} x {}'.format(size_x, size_y))
  terms = []
  for y in range(size_y):
    for x in range(size_x):
      s = x + size_x * y
      sx = (x + 1) % size_x + size_x * y
      sy = x + size_x * ((y + 1) % size_y)
      sxy = (x + 1) % size_x + size_x * ((y + 1) % size_y)
      terms.append((s, sx, sy, sxy))
      terms.append((s, sy, sx, sxy))
  return np.ascontiguousarray(np.asarray(terms, dtype=np.int32))


def check_four_spin_terms(terms, n_sites=None):
  """[n_terms][4] int32 of `terms`, or ValueError: every term names four distinct sites (in 0 .. n_sites - 1 where
  n_sites is given)."""
  t = np.asarray(terms)
  if t.size == 0 or t.ndim != 2 or t.shape[1] != 4 or not np.issubdtype(t.dtype, np.integer):
    raise ValueError('four-spin terms: a list of (i, j, k, l) integer site indices required, got shape {}'.format(t.shape))
  for k, row in enumerate(t):
    if len(set(int(s) for s in row)) != 4 or row.min() < 0 or (n_sites is not None and row.max() >= n_sites):
      raise ValueError('four-spin term {} = {}: four distinct sites{} required'.format(
          k, tuple(int(s) for s in row), '' if n_sites is None else ' in 0 .. {}'.format(n_sites - 1)))
  return np.ascontiguousarray(t.astype(np.int32))


def read_four_spin_terms(path, default_q=1.0):
  """(terms [n][4] int32, q [n] float32) from a text file of rows `i j k l [q]`: blanks or commas separate, `#` starts a
  comment, a line without any field is skipped; a row without a fifth column takes default_q."""
  terms, q = [], []
  with open(path) as f:
    for number, line in enumerate(f, 1):
      fields = line.split('#', 1)[0].replace(',', ' ').split()
      if not fields:
        continue
      try:
        sites = [int(x) for x in fields[:4]]
        value = float(fields[4]) if len(fields) == 5 else float(default_q)
      except ValueError:
        sites = []
      if len(sites) != 4 or len(fields) > 5 or not np.isfinite(value):
        raise ValueError('{}:{}: a line is a four-spin term `i j k l [q]` of integer site indices and a finite coupling, '
                         'got {!r}'.format(path, number, line.strip()))
      terms.append(sites)
      q.append(value)
  if not terms:
    raise ValueError('{}: no four-spin term'.format(path))
  return check_four_spin_terms(np.asarray(terms, dtype=np.int64)), np.asarray(q, dtype=np.float32)


def write_four_spin_terms(path, terms, q=None):
  """Rows `i j k l` (q None) or `i j k l q` (a scalar or one value per term) for read_four_spin_terms."""
  terms = check_four_spin_terms(terms)
  values = None if q is None else np.broadcast_to(np.asarray(q, np.float64), (terms.shape[0],))
  with open(path, 'w') as f:
    for k, (a, b, c, d) in enumerate(terms):
      f.write('{} {} {} {}'.format(a, b, c, d) + ('\n' if values is None else ' {!r}\n'.format(float(values[k]))))


def load_four_spin_terms(checkpoint_dir, default_q=1.0):
  """(terms, q) of `Q.txt` in a run directory, or None when the directory has none."""
  path = os.path.join(checkpoint_dir, 'Q.txt')
  if not os.path.exists(path):
    return None
  return read_four_spin_terms(path, default_q)

"""The inputs of the symmetrized shape tests (tests/test_gpu_symmetrized_shapes.py): lattices, op sets, sectors and seeds.
One place, importable without a GPU, so that tests/test_symmetrized.py proves on the fp64 oracle alone what the GPU tests
take for granted: every op set is a set of symmetries of its bonds, the fold identity holds on it, the sign sector of the
space group is a representation, and the batches of the gradient tests keep min_c r >= 0.01.

What each shape reaches in csrc/symz.hip (tests/test_gpu_symmetrized.py stays on the 8-site chain and the 4 x 4 torus):
  chain10       N % 4 = 2: the `i < N` guard inside k_symz_accept's last Philox block of four
  chain12       translations times the spin flip off the 8-site chain
  chain68       N > 64, a multiple of 4: the second trip of k_symz_candidates' `i += 64` site loop (and k_symm_rows')
  chain70       N > 64 and N % 4 = 2: both at once
  chain258      (N + 3) / 4 = 65 Philox blocks, the last one short: lane 0's second trip of k_symz_accept's block loop
  torus6x4      a rectangle: translations whose two periods differ
  torus4-sg     the space group of the 4 x 4 torus, 8 point-group ops x 16 translations: 128 ops that do not commute
  torus4-j1j2   the same ops under two couplings (J2 = 0.5 J1 on the diagonal bonds): plan_symm_check_hamiltonian's
                per-bond comparison, the fold identity with couplings that differ by bond
  chain20       an ed_vector base of 184,756 entries (a random vector: no diagonalisation)
"""
import functools

import numpy as np

from cgs_vmc_amd import lattice
from oracle import vmc_oracle as vo
from tests import symmetrized_oracle as so

SEED = 2024                                    # the engines' sampler seed
ZERO_R = 1e-12                                 # tests/test_gpu_symmetrized.py's: the oracle's r at a structural zero
R_MIN = 0.01                                   # the smallest cancellation a gradient batch may hold


def _chain(n):
  return dict(n=n, sx=n, sy=1, bonds=vo.chain_bonds(n), j=1.0)


J2 = 0.5
LATTICES = {
    'chain8': _chain(8), 'chain10': _chain(10), 'chain12': _chain(12), 'chain20': _chain(20), 'chain68': _chain(68),
    'chain70': _chain(70), 'chain258': _chain(258),
    'torus6x4': dict(n=24, sx=6, sy=4, bonds=vo.torus_bonds(6, 4), j=1.0),
    'torus4': dict(n=16, sx=4, sy=4, bonds=vo.torus_bonds(4, 4), j=1.0),
    # 32 nearest-neighbour bonds at J1 = 1, then 32 diagonal ones at J2: one coupling per bond
    'torus4-j1j2': dict(n=16, sx=4, sy=4, bonds=vo.torus_bonds(4, 4, next_nearest=True),
                        j=np.r_[np.ones(32), np.full(32, J2)].astype(np.float32)),
}

# the one-dimensional representations of C4v in lattice.point_group's order (identity, rot90, rot180, rot270, mirror_x,
# mirror_y, mirror_diag, mirror_antidiag), at momentum (0, 0): a character of the space group depends on the point-group
# part of an op alone.  'sign' is B1 (rotations by 90 degrees and the diagonal mirrors odd); A2 has every mirror odd.
POINT_SIGNS = {
    'trivial': [+1, +1, +1, +1, +1, +1, +1, +1],
    'sign': [+1, -1, +1, -1, +1, +1, -1, -1],
    'A2': [+1, +1, +1, +1, -1, -1, -1, -1],
}


@functools.lru_cache(maxsize=None)
def space_group(sx, sy):
  """(perms [n_pg * N][N], point-group index per op): op p N + t reads row[i] = x[pg_p[t[i]]] -- a translation, then the
  point-group op p about site 0.  The identity comes first."""
  _, pg = lattice.point_group(sx, sy)
  tr = lattice.translations(sx, sy)
  perms = np.ascontiguousarray(np.stack([p[t] for p in pg for t in tr]).astype(np.int32))
  return perms, np.repeat(np.arange(len(pg)), len(tr))


@functools.lru_cache(maxsize=None)
def ops(lat, sector):
  """(perms int32 [n_ops][N], flips uint8 [n_ops] or None, chi float64 [n_ops]) of a named sector:
    q<m> / q<mx>,<my>      lattice.sector_characters over the translations; a trailing + / -: times the global spin flip
    sub<d>                 the translations by multiples of d sites along x, trivial sector
    sg-<name>              the space group of a square torus with the point-group signs POINT_SIGNS[name]
  validated by lattice.check_symmetry_ops and, against the lattice's bonds, lattice.check_hamiltonian_symmetry."""
  L = LATTICES[lat]
  flips = None
  if sector.startswith('sg-'):
    perms, pg_of = space_group(L['sx'], L['sy'])
    chi = np.asarray(POINT_SIGNS[sector[3:]], np.float64)[pg_of] / len(perms)
  elif sector.startswith('sub'):
    step = int(sector[3:])
    assert L['sx'] % step == 0
    perms = lattice.translations(L['sx'], L['sy'])[[r for r in range(L['sx']) if r % step == 0]]
    chi = np.full(len(perms), 1.0 / len(perms))
  else:
    spin_flip = sector[-1] in '+-'
    perms = lattice.translations(L['sx'], L['sy'])
    labels, table = lattice.sector_characters(L['sx'], L['sy'], spin_flip=spin_flip)
    chi = table[labels.index(sector)]
    if spin_flip:
      perms, flips = np.concatenate([perms, perms]), np.repeat([0, 1], len(perms)).astype(np.uint8)
  perms, checked = lattice.check_symmetry_ops(perms, flips, L['n'])
  lattice.check_hamiltonian_symmetry(L['bonds'], L['j'], L['j'], perms)
  assert len({p.tobytes() + bytes([f]) for p, f in zip(perms, checked)}) == len(perms)      # the ops are distinct
  chi = np.ascontiguousarray(chi, np.float64)
  for a in (perms, chi) + (() if flips is None else (checked,)):
    a.setflags(write=False)
  return perms, (None if flips is None else checked), chi


def couplings(lat, jx=1.0, jz=1.0):
  """(j_x, j_z) of a lattice: its per-bond pattern times the two factors."""
  j = LATTICES[lat]['j']
  return np.float32(jx) * np.asarray(j, np.float32), np.float32(jz) * np.asarray(j, np.float32)


def configs(n, b, seed, oracle=None):
  """tests/test_gpu_symmetrized.py's _configs: b random Sz = 0 rows of the seeded stream; with an oracle the first b that
  are at no structural zero of its sector."""
  cfg = vo.random_configurations(n, 16 * b + 256, np.random.RandomState(seed))
  if oracle is not None:
    cfg = cfg[oracle.cancellation(cfg) > ZERO_R]
  assert len(cfg) >= b
  return np.ascontiguousarray(cfg[:b])


# ---- 1. amplitudes and local energies: (base kind, lattice, sector, chains)
AMPLITUDE_CASES = [
    ('fc2x16', 'chain10', 'q5', 5), ('fc2x16', 'chain12', 'q0-', 5), ('fc2x16', 'chain68', 'q34', 5),
    ('fc2x16', 'chain70', 'q35', 5), ('fc2x16', 'chain258', 'sub43', 5), ('fc2x16', 'torus6x4', 'q3,2', 5),
    ('fc2x16', 'torus4', 'sg-trivial', 5), ('fc2x16', 'torus4', 'sg-sign', 5), ('fc2x16', 'torus4-j1j2', 'sg-sign', 5),
    ('pbdg', 'chain68', 'q34', 5), ('edvec', 'chain20', 'q10', 5), ('rbm', 'chain70', 'q0-', 3)]
AMPLITUDE_SEED, ELOC_SEED = 21, 26             # tests/test_gpu_symmetrized.py's batch seeds for the two checks

# ---- 2. more than one fold workgroup, more than one trip of the row kernels
BIG = dict(lat='chain68', sector='q34', b=260, seed=41, step_seed=42)
ROW_ITEMS_PER_CU = 16 * 4                      # measure_dev.hpp measure_rows_grid: at most 16 blocks of 4 items per CU
FOLD_THREADS = 256                             # plan.hpp PLAN_SYMZ_THREADS
BAND_SHARE = 0.02


def big_step(cfg):
  """(i_up, i_dn, u) of the big case's one injected step: a random up site to lower and down site to raise per chain."""
  rng = np.random.default_rng(BIG['step_seed'])
  i_up = np.array([rng.choice(np.flatnonzero(row > 0)) for row in cfg], np.int32)
  i_dn = np.array([rng.choice(np.flatnonzero(row < 0)) for row in cfg], np.int32)
  return i_up, i_dn, rng.random(len(cfg)).astype(np.float32)

# ---- 3. the in-kernel proposal draw: (lattice, sector); B = 5, chain offsets 0 and 11, four steps
DRAW_CASES = [('chain8', 'q4'), ('chain70', 'q35'), ('chain258', 'sub43')]
DRAW_OFFSETS = (0, 11)
DRAW_SEED = 27
HIGH_STEP = 2 ** 33 + 1

# ---- 4. the fold alone: last-layer factors chosen on the oracle (test_symmetrized.py asserts the spreads they give)
FOLD_CASES = [('chain10', 'q5'), ('chain70', 'q35')]
FOLD_SEED = 51
# factor -> the spread max_k l_k - min_k l_k that EVERY row's orbit must exceed.  At factor 1 the smallest spread of the
# ten rows is 0.233 (chain10; 0.929 on chain70), so 500 gives 116 .. 597 -- past fp32's exp range, inside fp64's -- and 4000
# gives 932 .. 5724: past fp64's, the far terms underflow to exactly 0
FOLD_FACTORS = {1.0: 0.0, 500.0: 88.0, 4000.0: 745.0}


def fold_theta(n, factor, bias=0.0):
  """init_params(seed 0) of the 2 x 16 network with the last layer's 16 weights times `factor` -- the logits scale by it --
  and the output bias `bias` (0 at init)."""
  theta = vo.init_params(n, 16, 2, np.random.default_rng(0)).astype(np.float64)
  assert theta[-1] == 0.0
  theta[-17:-1] *= factor
  theta[-1] = bias
  return theta.astype(np.float32)


def orbit_logits(theta, oracle, cfg):
  """[n_ops][B] fp64 logits of the 2 x 16 network on the permuted rows."""
  rows = oracle.rows(cfg)
  k, b, n = rows.shape
  return vo.fc_logit(np.asarray(theta, np.float64), rows.reshape(k * b, n), 16, 2, dtype=np.float64).reshape(k, b)


def host_fold(logit, chi, sign=None):
  """symz_sum in numpy fp64 on [n_ops][B] logits: ops ascending, max shift over the ops that count -> (m + ln|S|, sgn S, r).
  np.exp underflows to exactly 0 below -745, as the kernel's exp does."""
  logit = np.asarray(logit, np.float64)
  chi = np.asarray(chi, np.float64)
  sign = np.ones_like(logit) if sign is None else np.asarray(sign, np.float64)
  counts = (chi[:, None] != 0) & (sign != 0) & ~np.isneginf(logit)
  m = np.where(counts, logit, -np.inf).max(0)
  s, a = np.zeros(logit.shape[1]), np.zeros(logit.shape[1])
  for k in range(len(chi)):
    with np.errstate(under='ignore', invalid='ignore'):
      e = np.where(counts[k], np.exp(logit[k] - m), 0.0)
    s += chi[k] * np.sign(sign[k]) * e
    a += abs(chi[k]) * e
  with np.errstate(divide='ignore'):
    return m + np.log(np.abs(s)), np.sign(s), np.abs(s) / a


# ---- 5. ops that do not count
ZERO_CHI_SEED = 61
# fold_theta's factor at which, on 2 of the 13 host rows, an odd translation's logit lies 1,090 above every even one's
ZERO_CHI_FACTOR = 8000.0
# q2 of the 8-site chain with the zeros it should have: cos(pi r / 2) is 1, 0, -1, 0, ... exactly; mult = 2 (k != -k)
CHI_Q2_EXACT = np.array([1, 0, -1, 0, 1, 0, -1, 0], np.float64) * 2.0 / 8.0
ZERO_AMP = dict(vector_seed=71, zero_share=0.3, sectors=('q0', 'q4'), b=5, pool_seed=72)
DOMAIN_WALL = np.array([1, 1, 1, 1, -1, -1, -1, -1], np.float32)      # its eight translates are all zeros of the vector


def zero_vector(n=8):
  """(float32 vector over the Sz = 0 configurations with about 30 % exact zeros -- by seed, and the whole translation
  orbit of DOMAIN_WALL --, top, bot)."""
  from tests import edvec_oracle as eo
  top, bot, length = eo.lin_tables(n)
  rng = np.random.default_rng(ZERO_AMP['vector_seed'])
  vec = (1.0 + 0.5 * rng.random(length)) * np.where(rng.random(length) < 0.2, -1.0, 1.0)
  vec[rng.random(length) < ZERO_AMP['zero_share']] = 0.0
  vec[eo.index(DOMAIN_WALL[lattice.translations(n)], top, bot)] = 0.0
  return vec.astype(np.float32), top, bot


def zero_amp_batch(oracle, n=8):
  """(batch [b][n], partial [b]): distinct rows of the seeded pool with psi_s != 0 in the oracle's sector; the rows with
  some but not all of their ops on a zero entry come first (partial marks them)."""
  b = ZERO_AMP['b']
  pool = vo.random_configurations(n, 400, np.random.RandomState(ZERO_AMP['pool_seed']))
  pool = pool[np.sort(np.unique(pool, axis=0, return_index=True)[1])]
  with np.errstate(invalid='ignore'):
    alive = oracle.cancellation(pool) > ZERO_R             # (0 / 0 where every op hits a zero: NaN, not alive)
  dead = (oracle.terms(pool) == 0).sum(0)
  partial = alive & (dead > 0) & (dead < oracle.n_ops)
  order = np.r_[np.flatnonzero(partial), np.flatnonzero(alive & ~partial)][:b]
  return np.ascontiguousarray(pool[order]), partial[order]


# ---- 6. gradient sums: (lattice, sector, chains) -> (theta seed, batch seed), searched on the oracle
# (tests/test_symmetrized.py::test_the_gradient_seed_table_keeps_r_min asserts each; the measured r_min beside it)
GRADIENT_SEEDS = {
    ('chain70', 'q35', 5): (0, 34),                 # r_min 0.0286
    ('torus4', 'sg-sign', 5): (0, 38),              # r_min 0.0125
    ('torus4-j1j2', 'sg-sign', 5): (0, 38),         # (the same ops and rows: r does not know the bonds)
    ('chain258', 'sub43', 5): (0, 31),              # r_min 1: the trivial sector of a positive state
}
GRADIENT_CASES = list(GRADIENT_SEEDS)


def fc_theta(n, theta_seed):
  """init_params of the 2 x 16 network (tests/test_gpu_symmetrized.py's _factor draws the same floats)."""
  return vo.init_params(n, 16, 2, np.random.default_rng(theta_seed))


def fc_oracle(lat, sector, theta):
  from tests import prod_oracle as pro
  perms, flips, chi = ops(lat, sector)
  return so.Symmetrized(pro.fc_factor(theta, 16, 2), perms, flips, chi)

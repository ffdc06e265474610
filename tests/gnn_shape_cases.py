"""The inputs of the gnn shape tests (tests/test_gpu_gnn_shapes.py) and the host-side arithmetic they lean on.  One place,
importable without a GPU, so that tests/test_gnn.py proves on the oracle alone what the GPU tests take for granted: the
tables have the properties their names promise, the sampler comparison keeps enough chains outside the tie band, and the
launches meant to cross a grid cap do cross it.

What each edge shape reaches in csrc/conv_general.hip / csrc/vmc_api_cgen.hip:
  single-layer    n_conv == 1: lda = (k + 3) & ~3, no backward through k_gnn_col2im
  ring-10         k = 2, the smallest table; F = 5: the scalar gathers
  wide-table-k64  k = PLAN_GNN_MAX_K
  deep-4          L = 4 (three col2im passes per backward), sigmoid, a table without forced self entries
  empty-lists-*   two sites in no row: ptr[n] == ptr[n + 1], their input gradient is 0; F = 8 / F = 6: VEC = 4 / 1
  hub-16          site 0 is read by every non-first tap: one inverse list of 65 entries next to lists of one
  split-k         M = rows N = 4096: cgen_weight_sums takes split-K off a graph's im2col matrix
"""
import functools

import numpy as np

from oracle import vmc_oracle as vo
from tests import gnn_oracle as go

SEED = 2024                                    # the engines' sampler seed
BAND = 1e-4                                    # | |psi'/psi| - sqrt(u) | < 1e-4 |psi'/psi|: a tie, not compared
STEPS = 12


@functools.lru_cache(maxsize=None)
def graph(name):
  """(adjacency [N, k], bonds) of a named table."""
  rng = np.random.default_rng(sum(map(ord, name)))
  if name.startswith('triangular-'):
    lx, ly = map(int, name.split('-')[1].split('x'))
    return go.triangular_adjacency(lx, ly), go.triangular_bonds(lx, ly)
  adj = {
      'honeycomb-18': lambda: go.honeycomb_adjacency(3, 3),
      'irregular-12': go.irregular_adjacency,
      'ring-10': lambda: go.ring_adjacency(10),
      'wide-20': lambda: go.random_adjacency(20, 64, rng, self_first=True),
      'random-30': lambda: go.random_adjacency(30, 6, rng),
      'empty-14': lambda: go.empty_list_adjacency(14, 5, 12, rng),
      'hub-16': lambda: go.hub_adjacency(16, 5),
  }[name]()
  return adj, go.adjacency_bonds(adj)


# parameters and start chains: seeds 3 / 4 (tests/test_gpu_gnn.py's) for every case; with them the oracle's 12 steps keep
# at least three quarters of the chains outside the tie band
# (tests/test_gnn.py::test_gnn_edge_cases_keep_three_quarters_of_the_chains_outside_the_tie_band)
EDGE_CASES = {
    'single-layer': dict(graph='triangular-4x4', L=1, f=10, b=17, nonlin='relu'),
    'ring-10': dict(graph='ring-10', L=3, f=5, b=11, nonlin='tanh'),
    'wide-table-k64': dict(graph='wide-20', L=2, f=4, b=6, nonlin='relu'),
    'deep-4': dict(graph='random-30', L=4, f=12, b=9, nonlin='sigmoid', overlap=True),
    'empty-lists-F8': dict(graph='empty-14', L=2, f=8, b=13, nonlin='tanh', overlap=True),
    'empty-lists-F6': dict(graph='empty-14', L=2, f=6, b=13, nonlin='relu'),
    'hub-16': dict(graph='hub-16', L=2, f=6, b=10, nonlin='cos'),
    'split-k': dict(graph='triangular-8x8', L=2, f=8, b=64, nonlin='relu'),
}
EDGE_IDS = list(EDGE_CASES)
# the two cases of tests/test_gpu_gnn.py that run again in several blocks
BLOCK_CASES = {
    'irregular-12': dict(graph='irregular-12', L=3, f=6, b=18, nonlin='cos'),
    'honeycomb-18': dict(graph='honeycomb-18', L=2, f=64, b=20, nonlin='tanh', oact='identity'),
}


def inputs(case):
  """theta, the start chains, the table and the bonds of a case dict (tests/test_gpu_gnn.py's recipe)."""
  adj, bonds = graph(case['graph'])
  n, k = adj.shape
  f = case['f']
  theta = go.gnn_init_params(k, f, case['L'], np.random.default_rng(3),
                             noise=0.03 if f <= 16 else 0.01)
  cfg = vo.random_configurations(n, case['b'], np.random.RandomState(4))
  return theta, cfg, adj, bonds


def oracle_steps(theta, cfg, adj, f, L, nonlin, oact='exp', steps=STEPS, seed=SEED):
  """`steps` steps of the oracle's sampler on the engines' Philox streams: (chains, ok), ok[c] False once chain c
  came within BAND of a tie."""
  amp = lambda c: go.gnn_psi(theta, c, adj, f, L, -10.0, nonlin, oact)
  b, n = cfg.shape
  cur, ok = cfg, np.ones(b, bool)
  for step in range(steps):
    u_sites, u_acc = vo.step_uniforms(seed, np.arange(b), step, n)
    i_up, i_dn = vo.propose_exchange(cur, u_sites)
    cur, _, ratios = vo.mc_step(amp, cur, i_up, i_dn, u_acc)
    ok &= ~(np.abs(ratios - np.sqrt(u_acc.astype(np.float64))) < BAND * np.maximum(ratios, 1e-30))
  return cur, ok


# ---------------------------------------------------------------------------- random graphs
ACTS = ['relu', 'tanh', 'sigmoid', 'identity', 'cos']


def random_graph_shapes(count, seed=6066):
  """Seeded random tables, alternating narrow (1 .. 13 filters) and wide (64 .. 100): an even number of sites in 4 .. 60,
  2 .. 12 taps uniform over the sites (self not forced), 1 .. 3 layers, 1 .. 24 chains; a table without a bond is skipped.
  Yields (sites, taps, filters, layers, chains, nonlinearity, table_seed)."""
  rng = np.random.default_rng(seed)
  shapes = []
  while len(shapes) < count:
    wide = len(shapes) % 2 == 1
    n = 2 * int(rng.integers(2, 31))
    k = int(rng.integers(2, 13))
    f = int(rng.integers(64, 101)) if wide else int(rng.integers(1, 14))
    L = int(rng.integers(1, 4))
    b = int(rng.integers(1, 25))
    nonlin = ACTS[int(rng.integers(len(ACTS)))]
    table_seed = int(rng.integers(1 << 30))
    if not go.adjacency_bonds(random_table(n, k, table_seed)):
      continue
    shapes.append((n, k, f, L, b, nonlin, table_seed))
  return shapes


def random_table(n, k, table_seed):
  return go.random_adjacency(n, k, np.random.default_rng(table_seed))


def random_graph_inputs(n, k, f, L, b):
  """theta and start chains of a random shape.  The logit sums N F entries of the last map, each of order one at
  snt.Conv2D's init, so its spread grows as sqrt(N F): at 46 sites x 72 filters the amplitude ratios of the connected
  configurations reach e^90 and the weighted gradient sum leaves fp32's range in the ORACLE (3.9e39).  The last layer is
  scaled so that the logits stay at the magnitudes of tests/test_gpu_gnn.py's shapes (N F = 128), as
  tests/test_gpu_conv.py's _make scales its noise to the fan-in."""
  rng = np.random.default_rng(b + 7 * k)
  theta = go.gnn_init_params(k, f, L, rng, noise=0.03 if f <= 16 else 0.01)
  last = k * (f if L > 1 else 1) * f + f
  theta[-last:] *= np.float32(min(1.0, np.sqrt(128.0 / (n * f))))
  cfg = vo.random_configurations(n, b, np.random.RandomState(b + 7 * k + 1))
  return theta, cfg


RANDOM_GRAPHS = random_graph_shapes(12)


# ---------------------------------------------------------------------------- chain groups, step tail
SAMPLER_CASES = [
    dict(graph='triangular-6x6', L=2, f=8, b=9, nonlin='relu', tail=True),
    dict(graph='honeycomb-18', L=2, f=64, b=37, nonlin='tanh', tail=True),
    dict(graph='irregular-12', L=3, f=6, b=3, nonlin='cos', tail=False),          # fewer chains than groups
]

# ---------------------------------------------------------------------------- tile GEMM kernels under a stencil table
# torus side, filters, chains; K = 9 F of every convolution behind the first
STENCIL_TILE_CASES = [
    (8, 64, 16),       # K = 576 = 18 stages of 32: k_gemm_ring, not whole turns of its four-stage ring
    (6, 128, 16),      # K = 1152 = 36 stages: whole turns
    (6, 72, 16),       # K = 648, no multiple of 32: k_gemm128 where forced, one column tile clamped at 72 of 128
]
GEMM_MODES = ('0', '2', '5')                   # CGS_VMC_GEMM128: k_gemm everywhere / k_gemm128 / k_gemm_ring where they apply
# (restated constants of the sources: tests/test_gnn.py::test_gnn_shape_case_constants_are_the_sources reads each back)
GEMM_TILE_ROWS = 128                           # grad.hip `#define G2_TM`
GEMM_RING_MIN = 160                            # grad.hip `#define GEMM_RING_MIN`: tiles from which launch_gemm picks k_gemm_ring
SPLITK_MIN = 4096                              # vmc_api_cgen.hip cgen_weight_sums `m.splitk = M >= 4096 ? ...`

# ---------------------------------------------------------------------------- launches past the grid caps
CG_BLOCKS_CAP = 16384                          # conv_general.hip cg_blocks(): workgroups of 256 items
IM2COL_GRID_CAP = 65536                        # conv_general.hip launch_cgen_im2col `grid(blocks < 65536 ? ...)`: workgroups of ppb positions
SMALL = 64                                     # chains per reference engine
BIG_GRAPH = 'triangular-8x8'
BIG_L = 2
IM2COL_CASES = [dict(f=12, b=320), dict(f=6, b=320)]                       # VEC = 4 / the scalar form
# crosses: 4,227,072 items at F = 6; the vec-4 form has 1,056,768 at b = 8,256 (below the cap) and 4,202,496 at 32,832
COL2IM_CASES = [dict(f=6, b=11008, crosses=True), dict(f=8, b=8256, crosses=False), dict(f=8, b=32832, crosses=True)]


def balanced_configurations(n, b, rng):
  """b rows of n / 2 up and n / 2 down spins (vo.random_configurations' distribution without its Python loop)."""
  order = np.argsort(rng.random((b, n)), axis=1)
  return np.where(order < n // 2, -1.0, 1.0).astype(np.float32)


def big_inputs(f, b):
  adj, bonds = graph(BIG_GRAPH)
  n, k = adj.shape
  theta = go.gnn_init_params(k, f, BIG_L, np.random.default_rng(31))
  cfg = balanced_configurations(n, b, np.random.default_rng(32 + f))
  return theta, cfg, adj, bonds


def connected_rows(cfg, bonds):
  """Rows of one local-energy call: the antiparallel (chain, bond) pairs (vmc_last_connected_rows)."""
  return int(sum((cfg[:, i] != cfg[:, j]).sum() for i, j in bonds))


def im2col0_items(rows, n, k):
  return rows * n * k


def im2col_positions_cap(k, f):
  """Positions one k_cgen_im2col launch holds without looping: 65,536 workgroups of ppb (launch_cgen_im2col)."""
  items = k * (f // 4 if f % 4 == 0 else f)
  ppb = 1 if items >= 512 else -(-512 // items)
  return IM2COL_GRID_CAP * ppb


def col2im_items(rows, n, f):
  return rows * n * (f // 4 if f % 4 == 0 else f)


def cgen_lda(k, f, L):
  return (k * (f if L > 1 else 1) + 3) & ~3    # plan.hpp plan_cgen_lda with K = 1, KW = k


def cgen_block_rows(n, k, f, L, b, num_cus=256):
  """Rows per block of a gnn ctx (vmc_api.hip create_conv_general, no env hook set) on a chip of num_cus CUs."""
  rows = (768 << 20) // (n * cgen_lda(k, f, L) * 4)
  rows = max(1, min(rows, (1 << 30) // n, max(b, 65536)))
  if rows * n // 128 >= 2 * num_cus:
    rows = (rows * n // (128 * num_cus)) * 128 * num_cus // n
  return rows

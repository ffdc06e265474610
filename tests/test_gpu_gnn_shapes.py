"""GPU: the gnn ansatz past the three small graphs of tests/test_gpu_gnn.py -- its own kernels (k_cgen_im2col<., true>,
k_cgen_im2col0<true>, k_gnn_col2im, the dA = G W^T product of cgen_input_grad) at the shapes, block counts, chain groups,
GEMM tilings and launch sizes where a wrong stride, offset or loop step would show.  Inputs and host-side arithmetic:
tests/gnn_shape_cases.py (checked on the CPU by tests/test_gnn.py); reference: tests/gnn_oracle.py in fp64, conv_2d on the
periodic stencil, or sub-cap launches of the same ctx family.  Tolerances are those of tests/test_gpu_gnn.py and
tests/test_gpu_conv_general.py."""
import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import gnn_oracle as go
from tests import gnn_shape_cases as gsc
from tests.test_gpu_conv import _close
from tests.test_gpu_gnn import (_acc_close, _check_energy_gradient, _check_forward, _check_local_energy,
                                _check_log_overlap, _check_sampler_steps, _check_sr, _engine, _logits_close)

pytestmark = pytest.mark.gpu


def _run_case(case):
  """Amplitudes (chains and a second batch), local energies, 12 sampler steps, the EnergyGradient accumulators and, where
  the case asks for them, the LogOverlapITSWO accumulators, all against fp64."""
  theta, cfg, adj, bonds = gsc.inputs(case)
  L, f, b, nonlin, oact = case['L'], case['f'], case['b'], case['nonlin'], case.get('oact', 'exp')
  eng = _engine(adj, L, f, b, nonlin, oact)
  assert eng.kernel_path() == 6 and eng.num_params == theta.size == go.gnn_num_params(adj.shape[1], f, L)
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, -1.0, 1.0)
  _check_forward(eng, theta, cfg, adj, f, L, nonlin, b2=13 if b != 13 else 7)
  _check_local_energy(eng, theta, cfg, adj, bonds, f, L, nonlin, oact, scaled=True)
  got = _check_sampler_steps(eng, theta, cfg, adj, f, L, nonlin, oact)
  _check_energy_gradient(eng, theta, got, adj, bonds, f, L, nonlin, oact)
  if case.get('overlap'):
    theta_w = (theta + 0.02 * np.random.default_rng(17).standard_normal(theta.size)).astype(np.float32)
    _check_log_overlap(eng, theta, theta_w, got, adj, bonds, f, L, nonlin, oact)
  eng.close()


# ---------------------------------------------------------------------------- 1. edge shapes
@pytest.mark.parametrize('cid', gsc.EDGE_IDS)
def test_gnn_edge_shapes_fp64_parity(cid):
  case = gsc.EDGE_CASES[cid]
  if cid == 'split-k':
    assert case['b'] * gsc.graph(case['graph'])[0].shape[0] >= gsc.SPLITK_MIN
  _run_case(case)


# ---------------------------------------------------------------------------- 2. random graphs
@pytest.mark.parametrize('n,k,f,L,b,nonlin,table_seed', gsc.RANDOM_GRAPHS,
                         ids=['N{}-k{}-F{}-L{}-B{}-{}'.format(*s_[:6]) for s_ in gsc.RANDOM_GRAPHS])
def test_gnn_random_graphs(n, k, f, L, b, nonlin, table_seed):
  """tests/test_gpu_conv_general.py::test_general_convolution_random_shapes on random tables: amplitudes, local energies,
  the gradient sums and one injected mc_step with its tie band."""
  adj = gsc.random_table(n, k, table_seed)
  bonds = go.adjacency_bonds(adj)
  theta, cfg = gsc.random_graph_inputs(n, k, f, L, b)
  eng = _engine(adj, L, f, b, nonlin)
  assert eng.kernel_path() == 6 and eng.num_params == theta.size
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, -1.0, 1.0)
  amp = lambda c: go.gnn_psi(theta, c, adj, f, L, -10.0, nonlin)
  _logits_close(eng.amplitude()[0], theta, cfg, adj, f, L, nonlin)
  _check_local_energy(eng, theta, cfg, adj, bonds, f, L, nonlin, 'exp', scaled=True)
  acc = vo.Accumulators(theta.size, np.float64)
  e_ref = go.energy_gradient_accumulate(acc, theta, cfg, bonds, -1.0, 1.0, -10.0, adj, f, L, nonlin)
  assert np.abs(e_ref).max() < 1e12                # (the inputs: the weighted sums stay far inside fp32's range)
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  _acc_close(eng.get_accumulators(), acc, theta.size)
  u_sites, u_acc = vo.step_uniforms(5, np.arange(b), 0, n)
  i_up, i_dn = vo.propose_exchange(cfg, u_sites)
  _, acc_ref, ratios = vo.mc_step(amp, cfg, i_up, i_dn, u_acc)
  mask = eng.mc_step_injected(i_up, i_dn, u_acc)
  band = np.abs(ratios - np.sqrt(u_acc.astype(np.float64))) < gsc.BAND * np.maximum(ratios, 1e-30)
  assert np.array_equal(mask[~band], acc_ref[~band])
  eng.close()


# ---------------------------------------------------------------------------- 3. several blocks
@pytest.mark.parametrize('cid', list(gsc.BLOCK_CASES))
@pytest.mark.parametrize('block_rows', [5, 16])
def test_gnn_in_several_blocks(monkeypatch, block_rows, cid):
  """CGS_VMC_CONV_GENERAL_BLOCK_ROWS (read when the ctx is made) cuts every row loop of the path into blocks of 5 / 16
  rows: amplitudes, the local energies' rows, the sampler's candidates (several blocks: the four-launch step) and the
  gradient sums block by block -- cg_A, the tape and k_gnn_col2im's output rewritten per block.  The second batch of 13
  rows ends in a ragged block in every combination; the chains, and with them the gradient sums, do so in every one but
  the honeycomb's 20 chains at 5 rows (four whole blocks) -- irregular-12's 18 chains are 3 x 5 + 3 and 16 + 2."""
  monkeypatch.setenv('CGS_VMC_CONV_GENERAL_BLOCK_ROWS', str(block_rows))
  case = dict(gsc.BLOCK_CASES[cid], overlap=True)
  assert case['b'] > block_rows and 13 % block_rows
  assert (case['b'] % block_rows != 0) == ((cid, block_rows) != ('honeycomb-18', 5))
  _run_case(case)


@pytest.mark.parametrize('keep_tape', [None, '0'])
def test_gnn_stochastic_reconfiguration_in_blocks_of_five_rows(monkeypatch, keep_tape):
  """The body of tests/test_gpu_gnn.py::test_gnn_stochastic_reconfiguration with the 32 stored chains in seven blocks:
  the two-pass matvec (phase 2 re-runs forward and backward of every block, cg_sr_tape_rows reset between them), col2im
  in every block of every CG iteration; with CGS_VMC_SR_KEEP_TAPE unset and 0 (several blocks never keep a tape)."""
  monkeypatch.setenv('CGS_VMC_CONV_GENERAL_BLOCK_ROWS', '5')
  if keep_tape is None:
    monkeypatch.delenv('CGS_VMC_SR_KEEP_TAPE', raising=False)
  else:
    monkeypatch.setenv('CGS_VMC_SR_KEEP_TAPE', keep_tape)
  _check_sr(*gsc.graph('irregular-12'))


# ---------------------------------------------------------------------------- 4. chain groups, step tail
def _sampler_engine(case):
  theta, cfg, adj, bonds = gsc.inputs(case)
  eng = _engine(adj, case['L'], case['f'], case['b'], case['nonlin'])
  assert eng.kernel_path() == 6
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, -1.0, 1.0)
  return eng, cfg, adj.shape[0]


def _sample(eng, cfg, first, second):
  eng.set_configs(cfg)
  eng.step_counter = 0
  acc1 = eng.mc_steps(first)
  c1 = eng.get_configs()
  acc2 = eng.mc_steps(second)
  return acc1, c1, acc2, eng.get_configs(), eng.amplitude()[0]


SAMPLER_IDS = ['{graph}-F{f}-B{b}'.format(**c) for c in gsc.SAMPLER_CASES]


@pytest.mark.parametrize('case', gsc.SAMPLER_CASES, ids=SAMPLER_IDS)
def test_gnn_sampler_chain_groups_leave_the_chains_alone(monkeypatch, case):
  """tests/test_gpu_conv_general.py::test_sampler_chain_groups_leave_the_chains_alone on a gnn ctx, whose every convolution
  writes the explicit im2col matrix at the group's offset into cg_A (cg_map_row0): accept counts, the chains after 5 and
  after N more steps and the cached logits are the same bits for G = 1, 2, 3, 4."""
  eng, cfg, n = _sampler_engine(case)
  out = {}
  for groups in ('1', '2', '3', '4'):
    monkeypatch.setenv('CGS_VMC_CONV_GENERAL_GROUPS', groups)
    out[groups] = _sample(eng, cfg, 5, n)
  assert 0 < out['1'][2] <= n * case['b']
  for groups in ('2', '3', '4'):
    for a, bb in zip(out['1'], out[groups]):
      np.testing.assert_array_equal(a, bb)
  eng.close()


@pytest.mark.parametrize('case', [c for c in gsc.SAMPLER_CASES if c['tail']], ids=SAMPLER_IDS[:2])
def test_gnn_step_tail_launch_gives_the_chains_of_the_four_launches(monkeypatch, case):
  """CGS_VMC_CONV_STEP_TAIL=0 against unset: the same outputs, bit for bit."""
  eng, cfg, n = _sampler_engine(case)
  monkeypatch.setenv('CGS_VMC_CONV_STEP_TAIL', '0')
  four = _sample(eng, cfg, 5, n)
  monkeypatch.delenv('CGS_VMC_CONV_STEP_TAIL')
  one = _sample(eng, cfg, 5, n)
  assert 0 < one[2] <= n * case['b']
  for a, bb in zip(four, one):
    np.testing.assert_array_equal(a, bb)
  eng.close()


# ---------------------------------------------------------------------------- 5. tile GEMM kernels
def _stencil_pair(monkeypatch, side, f, b, L):
  """conv_2d K = 3 on a side x side torus and the gnn ctx on its stencil table, both on the explicit im2col + GEMM form."""
  from cgs_vmc_amd.engine import VmcEngine
  for key, v in (('CGS_VMC_CONV_GENERAL', '1'), ('CGS_VMC_CONV_BAND', '0'), ('CGS_VMC_CONV_GENERAL_IMPLICIT', '0'),
                 ('CGS_VMC_CONV_PATCH', '0')):
    monkeypatch.setenv(key, v)
  n, k = side * side, 3
  adj = go.stencil_adjacency(side, side, k)
  theta = vo.conv_init_params('conv_2d', (f, k, side, side), L, np.random.default_rng(0))
  noise = min(0.03, 0.03 * np.sqrt(400.0 / (f * k * k)))         # (tests/test_gpu_conv.py _make: scaled to the fan-in)
  theta += (noise * np.random.default_rng(1).standard_normal(theta.size)).astype(np.float32)
  cfg = vo.random_configurations(n, b, np.random.RandomState(2))
  bonds = vo.torus_bonds(side, side)
  engines = (VmcEngine(n, b, L, f, ansatz='conv_2d', kernel_size=k, size_x=side, size_y=side, seed=2024),
             _engine(adj, L, f, b, 'relu'))
  for eng in engines:
    assert eng.kernel_path() == 6
    eng.set_params(theta); eng.set_bonds(bonds, -1.0, 1.0)
  return engines, theta, cfg, adj, bonds


def _stencil_outputs(eng, cfg, steps):
  eng.set_configs(cfg)
  eng.step_counter = 0
  logit = eng.amplitude()[0]
  eloc = eng.local_energy()[0]
  eng.mc_steps(steps)
  chains = eng.get_configs()
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  return logit, eloc, chains, eng.amplitude()[0], eng.get_accumulators()


def _stencil_compare(conv, gnn, p):
  for a, bb in zip(conv[:4], gnn[:4]):
    np.testing.assert_array_equal(bb, a)
  a0, a1 = conv[4], gnn[4]
  for s in (slice(0, p), slice(p, 2 * p)):
    assert np.abs(a1[s] - a0[s]).max() <= 1e-5 * np.abs(a0[s]).max() + 1e-6
  np.testing.assert_array_equal(a1[2 * p:], a0[2 * p:])


@pytest.mark.parametrize('side,f,b', gsc.STENCIL_TILE_CASES, ids=['{0}x{0}-F{1}'.format(*c) for c in gsc.STENCIL_TILE_CASES])
def test_gnn_stencil_is_conv_2d_on_every_gemm_tiling(monkeypatch, side, f, b):
  """tests/test_gpu_gnn.py's stencil identity with the products forced onto k_gemm (CGS_VMC_GEMM128=0), k_gemm128 (2) and
  k_gemm_ring (5): the tile kernels read a graph's im2col matrix at lda = 9 F as they read the periodic one."""
  L = 2
  (conv, gnn), theta, cfg, adj, _ = _stencil_pair(monkeypatch, side, f, b, L)
  for mode in gsc.GEMM_MODES:
    monkeypatch.setenv('CGS_VMC_GEMM128', mode)
    out = [_stencil_outputs(eng, cfg, 2 * side * side) for eng in (conv, gnn)]
    _stencil_compare(out[0], out[1], theta.size)
    if mode == gsc.GEMM_MODES[-1]:
      _logits_close(out[1][0], theta, cfg, adj, f, L, 'relu')
  conv.close(); gnn.close()


def test_gnn_stencil_is_conv_2d_on_the_production_route(monkeypatch):
  """8 x 8, 64 filters, 64 chains, nothing forced on the products: the local-energy rows alone are more than GEMM_RING_MIN
  tiles (k_gemm_ring by launch_gemm's own rule), and the 4096 positions of the chains put the weight sums on split-K."""
  side, f, b, L = 8, 64, 64, 2
  (conv, gnn), theta, cfg, adj, bonds = _stencil_pair(monkeypatch, side, f, b, L)
  monkeypatch.delenv('CGS_VMC_GEMM128', raising=False)
  monkeypatch.delenv('CGS_VMC_GEMM_NARROW', raising=False)
  n = side * side
  assert gsc.connected_rows(cfg, bonds) * n // gsc.GEMM_TILE_ROWS >= gsc.GEMM_RING_MIN and b * n >= gsc.SPLITK_MIN
  assert (9 * f) % 32 == 0 and f >= 64                           # gemm_ring_ok
  out = [_stencil_outputs(eng, cfg, 2 * n) for eng in (conv, gnn)]
  assert gnn.last_connected_rows() * n // gsc.GEMM_TILE_ROWS >= gsc.GEMM_RING_MIN     # (the rows of the chains after the steps)
  _stencil_compare(out[0], out[1], theta.size)
  conv.close(); gnn.close()


# ---------------------------------------------------------------------------- 6. launches past the grid caps
def _small_engine(adj, f, bonds, theta):
  eng = _engine(adj, gsc.BIG_L, f, gsc.SMALL, 'relu')
  eng.set_params(theta); eng.set_bonds(bonds, -1.0, 1.0)
  return eng


def _subset_against_fp64(logit, eloc, theta, cfg, adj, bonds, f, seed):
  """A seeded subset of 64 chains of the large batch against the fp64 oracle."""
  pick = np.sort(np.random.default_rng(seed).choice(cfg.shape[0], gsc.SMALL, replace=False))
  sub = cfg[pick]
  _logits_close(logit[pick], theta, sub, adj, f, gsc.BIG_L, 'relu')
  amp = lambda c: go.gnn_psi(theta, c, adj, f, gsc.BIG_L, -10.0, 'relu')
  scale = go.gnn_forward(theta, sub, adj, f, gsc.BIG_L, 'relu', return_tape='scale')[1]
  _close(eloc[pick], vo.local_value(amp, sub, bonds, -1.0, 1.0, dtype=np.float64), max(2e-4, 4e-6 * float(scale.max())))


@pytest.mark.parametrize('case', gsc.IM2COL_CASES, ids=['F{f}-B{b}'.format(**c) for c in gsc.IM2COL_CASES])
def test_gnn_im2col_launches_past_their_grid_caps(case):
  """One local-energy call whose rows are ONE block (create_conv_general) and more than a launch of k_cgen_im2col0<true>
  (16,384 workgroups of 256 items) or k_cgen_im2col<., true> (65,536 workgroups of ppb positions) holds without looping:
  the grid-stride steps.  Reference: the same chains in engines of 64 -- every product at these filter counts is k_gemm,
  whose rows do not depend on the launch -- bit for bit, and a subset of 64 against fp64."""
  f, b = case['f'], case['b']
  theta, cfg, adj, bonds = gsc.big_inputs(f, b)
  n, k = adj.shape
  rows = gsc.connected_rows(cfg, bonds)
  assert gsc.im2col0_items(rows, n, k) > gsc.CG_BLOCKS_CAP * 256
  assert rows * n > gsc.im2col_positions_cap(k, f)
  assert rows <= gsc.cgen_block_rows(n, k, f, gsc.BIG_L, b)
  big = _engine(adj, gsc.BIG_L, f, b, 'relu')
  big.set_params(theta); big.set_configs(cfg); big.set_bonds(bonds, -1.0, 1.0)
  logit = big.amplitude()[0]
  eloc = big.local_energy()[0]
  assert big.last_connected_rows() == rows
  big.close()
  small = _small_engine(adj, f, bonds, theta)
  for r0 in range(0, b, gsc.SMALL):
    small.set_configs(cfg[r0:r0 + gsc.SMALL])
    np.testing.assert_array_equal(logit[r0:r0 + gsc.SMALL], small.amplitude()[0])
    np.testing.assert_array_equal(eloc[r0:r0 + gsc.SMALL], small.local_energy()[0])
  small.close()
  _subset_against_fp64(logit, eloc, theta, cfg, adj, bonds, f, seed=41)


@pytest.mark.parametrize('case', gsc.COL2IM_CASES, ids=['F{f}-B{b}'.format(**c) for c in gsc.COL2IM_CASES])
def test_gnn_col2im_launch_past_its_grid_cap(case):
  """One EnergyGradient accumulate whose chains are one block of the gradient path: k_gnn_col2im<1> at 11,008 chains x 64
  sites x 6 channels is 4,227,072 items against 16,384 workgroups of 256, so its grid-stride loop steps; k_gnn_col2im<4> at
  8,256 chains has 1,056,768 and does not, at 32,832 chains 4,202,496 and does.  Reference: the sum of the
  accumulators of the same chains in engines of 64, to the bound of test_gnn_sharded_chains_match_one_ctx; logits and local
  energies of every chain bit for bit; a subset of 64 against fp64."""
  f, b = case['f'], case['b']
  theta, cfg, adj, bonds = gsc.big_inputs(f, b)
  n, k = adj.shape
  assert (gsc.col2im_items(b, n, f) > gsc.CG_BLOCKS_CAP * 256) == case['crosses']
  assert b <= gsc.cgen_block_rows(n, k, f, gsc.BIG_L, b) and b % gsc.SMALL == 0
  big = _engine(adj, gsc.BIG_L, f, b, 'relu')
  big.set_params(theta); big.set_configs(cfg); big.set_bonds(bonds, -1.0, 1.0)
  logit = big.amplitude()[0]
  eloc = big.local_energy()[0]
  big.reset_accumulators()
  big.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  a = big.get_accumulators().astype(np.float64)
  big.close()
  small = _small_engine(adj, f, bonds, theta)
  s = np.zeros_like(a)
  first = None
  for r0 in range(0, b, gsc.SMALL):
    small.set_configs(cfg[r0:r0 + gsc.SMALL])
    small.reset_accumulators()
    small.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    part = small.get_accumulators()
    s += part
    first = part if first is None else first
    np.testing.assert_array_equal(logit[r0:r0 + gsc.SMALL], small.amplitude()[0])
    np.testing.assert_array_equal(eloc[r0:r0 + gsc.SMALL], small.local_energy()[0])
  small.close()
  p = theta.size
  assert np.abs(s[:2 * p] - a[:2 * p]).max() <= 1e-5 * np.abs(a[:2 * p]).max() + 1e-5
  assert abs(s[2 * p] - a[2 * p]) <= 1e-5 * abs(a[2 * p]) + 1e-5 and s[2 * p + 1] == a[2 * p + 1]
  # the reference engines against fp64 (their first 64 chains), the large batch's values on a seeded subset
  acc = vo.Accumulators(p, np.float64)
  go.energy_gradient_accumulate(acc, theta, cfg[:gsc.SMALL], bonds, -1.0, 1.0, -10.0, adj, f, gsc.BIG_L, 'relu')
  _acc_close(first, acc, p)
  _subset_against_fp64(logit, eloc, theta, cfg, adj, bonds, f, seed=43)

"""CPU: the gnn ansatz's front end (GraphConvNetwork, wavefunctions.py:1083-1154) -- registry, variable names and
shapes, adjacency-list validation, the C ABI's parameter count -- and the fp64 test oracle pinned to the periodic
one (tests/gnn_oracle.py on a stencil == oracle.conv_forward for conv_2d)."""
import copy
import os

import numpy as np
import pytest

from cgs_vmc_amd import session, utils, wavefunctions
from oracle import vmc_oracle as vo
from tests import gnn_oracle as go
from tests import gnn_shape_cases as gsc


def _hparams(tmp_path, adj, **kw):
  path = str(tmp_path / 'adjacency.txt')
  np.savetxt(path, np.asarray(adj), fmt='%d')
  kw.setdefault('num_sites', np.asarray(adj).shape[0])
  return utils.create_hparams(wavefunction_type='gnn', adjacency_list_path=path, **kw)


@pytest.mark.parametrize('num_layers', [1, 3])
def test_gnn_variables_names_and_shapes(tmp_path, num_layers):
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  adj = go.triangular_adjacency(3, 4)
  hp = _hparams(tmp_path, adj, num_conv_layers=num_layers, num_conv_filters=5)
  wf = wavefunctions.build_wavefunction(hp)
  assert isinstance(wf, wavefunctions.GraphConvNetwork)
  wf._n_sites = 12
  names, shapes = wf._shapes()
  expect_names, expect_shapes = [], []
  for l in range(num_layers):
    scope = 'graph_conv_network/graph_conv_layer' + ('' if l == 0 else '_%d' % l)
    expect_names += [scope + '/conv_2d/w', scope + '/conv_2d/b']
    expect_shapes += [(1, 7, 1 if l == 0 else 5, 5), (5,)]
  assert (names, shapes) == (expect_names, expect_shapes)
  assert wf.num_params == go.gnn_num_params(7, 5, num_layers)
  spec = wf._engine_spec()
  assert spec['ansatz'] == 'gnn' and spec['kernel_size'] == 7
  assert np.array_equal(np.frombuffer(spec['adjacency'], np.int32).reshape(12, 7), adj)
  dc = copy.deepcopy(wf)
  dc._n_sites = 12
  assert dc._shapes() == (['dc_' + n for n in expect_names], expect_shapes)
  assert dc._engine_spec() == spec                # psi and its supervisor copy share one ctx
  hash(tuple(sorted(spec.items())))
  other = wavefunctions.GraphConvNetwork(num_layers, 5, go.square_5point_adjacency(3, 4))
  assert other._engine_spec() != spec


def test_gnn_exp_normalization_and_output_activation(tmp_path):
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  adj = go.square_5point_adjacency(4, 4)
  wf = wavefunctions.build_wavefunction(_hparams(tmp_path, adj))
  assert wf._get_shift() == np.float32(-10.0)
  wf = wavefunctions.build_wavefunction(_hparams(tmp_path, adj, output_activation='identity'))
  assert wf._get_shift() is None


def test_gnn_malformed_adjacency_lists_raise(tmp_path):
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  good = go.square_5point_adjacency(4, 4)
  path = str(tmp_path / 'one_column.txt')
  np.savetxt(path, np.arange(16), fmt='%d')            # loads 1-D
  with pytest.raises(ValueError):
    wavefunctions.build_wavefunction(utils.create_hparams(wavefunction_type='gnn', adjacency_list_path=path,
                                                          num_sites=16))
  with pytest.raises(ValueError):                      # row count != num_sites
    wavefunctions.build_wavefunction(_hparams(tmp_path, good[:12], num_sites=16))
  for bad in (16, -1):                                 # entries outside [0, num_sites)
    adj = good.copy()
    adj[3, 2] = bad
    with pytest.raises(ValueError):
      wavefunctions.build_wavefunction(_hparams(tmp_path, adj))
  with pytest.raises(ValueError):                      # the table of another lattice size at connection
    wavefunctions.check_adjacency(good, 20)
  wf = wavefunctions.build_wavefunction(_hparams(tmp_path, good))
  assert isinstance(wf, wavefunctions.GraphConvNetwork)


def test_gnn_relative_path_is_read_from_the_working_directory(tmp_path, monkeypatch):
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  np.savetxt(str(tmp_path / 'adj.txt'), go.honeycomb_adjacency(2, 2), fmt='%d')
  monkeypatch.chdir(tmp_path)
  hp = utils.create_hparams(wavefunction_type='gnn', adjacency_list_path='adj.txt', num_sites=8,
                            checkpoint_dir=str(tmp_path / 'elsewhere'))
  wf = wavefunctions.build_wavefunction(hp)
  assert wf._kernel_size == 4


def test_gnn_num_params_c_abi():
  from cgs_vmc_amd import _hip
  if not os.path.exists(_hip.library_path()):
    import __graft_entry__ as g
    g.build()
  lib = _hip.load()
  assert _hip.ANSATZ_IDS['gnn'] == 6
  for L, f, k in ((1, 8, 7), (3, 16, 4), (2, 130, 64), (4, 5, 2)):
    assert lib.vmc_num_params_conv(6, L, f, k) == go.gnn_num_params(k, f, L) == \
        k * f + f + (L - 1) * (k * f * f + f)


@pytest.mark.parametrize('sx,sy,k,L,f,nonlin', [(4, 5, 3, 3, 6, 'tanh'), (6, 6, 5, 2, 4, 'relu'),
                                                 (5, 4, 4, 2, 3, 'cos')])
def test_gnn_oracle_on_the_stencil_is_the_conv_2d_oracle(sx, sy, k, L, f, nonlin):
  adj = go.stencil_adjacency(sx, sy, k)
  theta = vo.conv_init_params('conv_2d', (f, k, sx, sy), L, np.random.default_rng(0)).astype(np.float64)
  theta += 0.05 * np.random.default_rng(1).standard_normal(theta.size)
  cfg = vo.random_configurations(sx * sy, 9, np.random.RandomState(2))
  ref = vo.conv_forward(theta, cfg, 'conv_2d', (f, k, sx, sy), L, nonlin, np.float64)
  np.testing.assert_allclose(go.gnn_forward(theta, cfg, adj, f, L, nonlin), ref, rtol=1e-12, atol=1e-12)
  w = np.random.default_rng(3).standard_normal((9, 2))
  ref_g = vo.ANSATZ['conv_2d'][2](theta, cfg, w, (f, k, sx, sy), L, nonlin, np.float64)
  np.testing.assert_allclose(go.gnn_weighted_grads(theta, cfg, w, adj, f, L, nonlin), ref_g, rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------------------- the inputs of tests/test_gpu_gnn_shapes.py
def _all_tables():
  names = sorted({c['graph'] for c in list(gsc.EDGE_CASES.values()) + list(gsc.BLOCK_CASES.values()) + gsc.SAMPLER_CASES})
  tables = [(name, gsc.graph(name)[0]) for name in names + [gsc.BIG_GRAPH]]
  return tables + [('random-%d' % i, gsc.random_table(s[0], s[1], s[6])) for i, s in enumerate(gsc.RANDOM_GRAPHS)]


def test_gnn_shape_tables_are_in_range_and_keep_their_properties():
  for name, adj in _all_tables():
    n, k = adj.shape
    assert adj.dtype == np.int32 and 2 <= k <= 64 and n % 2 == 0, name
    assert adj.min() >= 0 and adj.max() < n, name
    wavefunctions.check_adjacency(adj, n)
    deg = go.in_degree(adj)
    assert deg.shape == (n,) and deg.sum() == n * k, name
    # the inverse lists (plan_gnn_inverse: entries m k + t of site s, position-major) have these lengths
    flat = adj.ravel()
    for s in range(n):
      assert deg[s] == np.flatnonzero(flat == s).size, (name, s)
    assert len(gsc.graph(name)[1] if not name.startswith('random-') else go.adjacency_bonds(adj)) > 0, name
  ring = gsc.graph('ring-10')[0]
  assert ring.tolist() == [[i, (i + 1) % 10] for i in range(10)]
  hub = gsc.graph('hub-16')[0]
  assert hub.shape == (16, 5) and (hub[:, 0] == np.arange(16)).all() and (hub[:, 1:] == 0).all()
  assert go.in_degree(hub).tolist() == [16 * 4 + 1] + [1] * 15          # a site read by almost every (position, tap)
  empty = gsc.graph('empty-14')[0]
  assert empty.shape == (14, 5) and (go.in_degree(empty)[12:] == 0).all() and (go.in_degree(empty)[:12] > 0).all()
  assert (empty[:12, 0] == np.arange(12)).all() and empty[12:].max() < 12    # rows 12 / 13 omit the site itself
  wide = gsc.graph('wide-20')[0]
  assert wide.shape == (20, 64) and (wide[:, 0] == np.arange(20)).all()
  deep = gsc.graph('random-30')[0]
  assert deep.shape == (30, 6) and (deep != np.arange(30)[:, None]).all(1).any()      # rows that omit the site itself
  assert gsc.graph('triangular-8x8')[0].shape == (64, 7)


def test_gnn_random_graph_shapes_cover_the_ranges():
  shapes = gsc.RANDOM_GRAPHS
  assert len(shapes) == 12 and shapes == gsc.random_graph_shapes(12)
  for i, (n, k, f, L, b, nonlin, _) in enumerate(shapes):
    assert n % 2 == 0 and 4 <= n <= 60 and 2 <= k <= 12 and 1 <= L <= 3 and 1 <= b <= 24 and nonlin in gsc.ACTS
    assert (64 <= f <= 100) if i % 2 else (1 <= f <= 13)
  assert {s[3] for s in shapes} == {1, 2, 3}
  for n, k, f, L, b, nonlin, table_seed in shapes:       # conditioning: logits and proposal ratios of moderate size
    theta, cfg = gsc.random_graph_inputs(n, k, f, L, b)
    adj = gsc.random_table(n, k, table_seed)
    assert theta.size == go.gnn_num_params(k, f, L) and cfg.shape == (b, n)
    assert np.abs(go.gnn_forward(theta, cfg, adj, f, L, nonlin)).max() < 60.0
    u_sites, u_acc = vo.step_uniforms(5, np.arange(b), 0, n)
    i_up, i_dn = vo.propose_exchange(cfg, u_sites)
    ratios = vo.mc_step(lambda c: go.gnn_psi(theta, c, adj, f, L, -10.0, nonlin), cfg, i_up, i_dn, u_acc)[2]
    assert 1e-8 < ratios.min() and ratios.max() < 1e8, (n, k, f, ratios.min(), ratios.max())
  assert any(s[2] % 4 for s in shapes) and any(s[2] % 4 == 0 for s in shapes)         # both VEC forms


@pytest.mark.parametrize('cid', gsc.EDGE_IDS + list(gsc.BLOCK_CASES))
def test_gnn_edge_cases_keep_three_quarters_of_the_chains_outside_the_tie_band(cid):
  """The GPU comparison of the 12 sampler steps leaves out chains within 1e-4 of a tie and asks that more than half
  remain; on the oracle alone at least three quarters do, so that cap cannot hide a failure."""
  case = gsc.EDGE_CASES.get(cid) or gsc.BLOCK_CASES[cid]
  theta, cfg, adj, _ = gsc.inputs(case)
  cur, ok = gsc.oracle_steps(theta, cfg, adj, case['f'], case['L'], case['nonlin'], case.get('oact', 'exp'))
  assert 4 * ok.sum() >= 3 * case['b'], (int(ok.sum()), case['b'])
  assert (cur.sum(1) == 0).all() and (cur != cfg).any()


def test_gnn_big_launches_cross_their_caps():
  """Item counts of the launches tests/test_gpu_gnn_shapes.py means to push past a grid cap, from the configurations and
  bonds alone; each is one block (create_conv_general's rule at 256 CUs)."""
  adj, bonds = gsc.graph(gsc.BIG_GRAPH)
  n, k = adj.shape
  for case in gsc.IM2COL_CASES:
    _, cfg, _, _ = gsc.big_inputs(case['f'], case['b'])
    assert cfg.shape == (case['b'], n) and (cfg.sum(1) == 0).all() and (np.abs(cfg) == 1).all()
    rows = gsc.connected_rows(cfg, bonds)
    assert gsc.im2col0_items(rows, n, k) > 16384 * 256
    assert rows * n > gsc.im2col_positions_cap(k, case['f'])
    assert rows <= gsc.cgen_block_rows(n, k, case['f'], gsc.BIG_L, case['b'])
  assert gsc.im2col_positions_cap(7, 12) == 65536 * 25 and gsc.im2col_positions_cap(7, 6) == 65536 * 13
  for case in gsc.COL2IM_CASES:
    items = gsc.col2im_items(case['b'], n, case['f'])
    assert (items > 16384 * 256) == case['crosses']
    assert case['b'] <= gsc.cgen_block_rows(n, k, case['f'], gsc.BIG_L, case['b']) and case['b'] % gsc.SMALL == 0
  assert gsc.col2im_items(11008, 64, 6) == 4227072 and gsc.col2im_items(8256, 64, 8) == 1056768 and gsc.col2im_items(32832, 64, 8) == 4202496
  assert gsc.cgen_lda(7, 12, 2) == 84 and gsc.cgen_lda(7, 10, 1) == 8 and gsc.cgen_block_rows(64, 7, 12, 2, 320) == 37376


def test_gnn_shape_case_constants_are_the_sources():
  """tests/gnn_shape_cases.py restates grid caps and thresholds that no entry of the C ABI reports; the 'past the cap'
  assertions of the GPU tests mean something only while the two agree, so each is read back out of the source line that
  sets it: whoever changes a cap there is sent to the test inputs."""
  csrc = os.path.join(os.path.dirname(os.path.abspath(wavefunctions.__file__)), 'csrc')
  read = lambda name: open(os.path.join(csrc, name)).read()
  general, grad, cgen, api = read('conv_general.hip'), read('grad.hip'), read('vmc_api_cgen.hip'), read('vmc_api.hip')
  cap = str(gsc.CG_BLOCKS_CAP)
  assert 'int cg_blocks(long long n) { const long long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b < %s ? b : %s)); }' % (cap, cap) in general
  assert 'const dim3 grid((unsigned)(blocks < %d ? blocks : %d));' % (gsc.IM2COL_GRID_CAP, gsc.IM2COL_GRID_CAP) in general
  assert 'const int ppb = (int)(items >= 512 ? 1 : (512 + items - 1) / items);' in general
  assert '#define GEMM_RING_MIN %d\n' % gsc.GEMM_RING_MIN in grad and '#define G2_TM %d\n' % gsc.GEMM_TILE_ROWS in grad
  assert 'm.splitk = M >= %d ? CGEN_SPLITK : 1;' % gsc.SPLITK_MIN in cgen
  # cgen_block_rows: the lines of create_conv_general it follows
  for line in ('long long block_mb = 768;',
               'if (rows > (1LL << 30) / cg.N) rows = (1LL << 30) / cg.N;',
               'if (rows > (B > 65536 ? B : 65536)) rows = B > 65536 ? B : 65536;',
               'if (rows * cg.N / 128 >= 2LL * c->num_cus) {',
               'rows = rounds * 128LL * c->num_cus / cg.N;'):
    assert line in api, line
  assert 'return (g.K * g.KW * (g.n_conv > 1 ? g.F : 1) + 3) & ~3; }' in read('plan.hpp')

"""GPU parity of the gnn ansatz -- GraphConvNetwork (wavefunctions.py:1083-1154; layers.GraphConvLayer,
layers.py:415-451) on the general convolution path's table-driven gathers (csrc/conv_general.hip) -- through the C
ABI and the training front end: bit-identity with conv_2d on a periodic stencil, fp64 parity (tests/gnn_oracle.py)
on triangular, honeycomb and irregular graphs, SR, sharded chains and run_training / run_energy_evaluation."""
import os

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import gnn_oracle as go
from tests import gnn_shape_cases as gsc
from tests.test_gpu_conv import _close

pytestmark = pytest.mark.gpu


_irregular_adjacency = go.irregular_adjacency


GRAPHS = {
    'triangular-4x4': (go.triangular_adjacency(4, 4), go.triangular_bonds(4, 4)),
    'honeycomb-18': (go.honeycomb_adjacency(3, 3), go.adjacency_bonds(go.honeycomb_adjacency(3, 3))),
    'irregular-12': (_irregular_adjacency(), go.adjacency_bonds(_irregular_adjacency())),
}
CASES = [
    # graph, num_layers, filters, batch, nonlinearity, output_activation
    ('triangular-4x4', 2, 8, 24, 'relu', 'exp'),
    ('honeycomb-18', 2, 64, 20, 'tanh', 'identity'),      # 64 filters: the implicit A-operand gather must refuse a graph
    ('irregular-12', 3, 6, 18, 'cos', 'exp'),             # filters % 4 != 0: the scalar gathers
]


def _engine(adj, L, f, b, nonlin, oact='exp', **kw):
  from cgs_vmc_amd.engine import VmcEngine
  return VmcEngine(adj.shape[0], b, L, f, nonlinearity=nonlin, output_activation=oact, ansatz='gnn',
                   adjacency=adj, seed=2024, **kw)


def _logits_close(got, theta, cfg, adj, f, L, nonlin):
  ref, scale = go.gnn_forward(theta, cfg, adj, f, L, nonlin, return_tape='scale')
  err = np.abs(np.asarray(got, np.float64) - ref)
  tol = 1e-6 * scale + 2e-5
  assert (err <= tol).all(), 'max err {} at {} (tol {})'.format(err.max(), err.argmax(), tol[err.argmax()])


def _acc_close(got, acc, p):
  for name, g, r in (('g1', got[:p], acc.g1_total), ('g2', got[p:2 * p], acc.g2_total)):
    tol = 2e-3 * np.abs(r).max() + 1e-4
    assert np.abs(g - r).max() < tol, (name, np.abs(g - r).max(), tol, int(np.argmax(np.abs(g - r))))


def test_gnn_on_the_periodic_stencil_is_conv_2d_bit_for_bit(monkeypatch):
  """The 3 x 3 stencil of a 6 x 6 torus as an adjacency list in cg_site's tap order IS conv_2d K = 3 with the same
  theta: on the explicit im2col + GEMM form of both, the same logits, local energies and chains, bit for bit; the
  gradient sums agree to fp32 (the graph's backward sums dA over inverse lists, conv_2d gathers transposed)."""
  from cgs_vmc_amd.engine import VmcEngine
  for k, v in (('CGS_VMC_CONV_GENERAL', '1'), ('CGS_VMC_CONV_BAND', '0'), ('CGS_VMC_CONV_GENERAL_IMPLICIT', '0'),
               ('CGS_VMC_CONV_PATCH', '0')):
    monkeypatch.setenv(k, v)
  sx = sy = 6
  n, L, f, b, k = 36, 3, 16, 32, 3
  adj = go.stencil_adjacency(sx, sy, k)
  theta = vo.conv_init_params('conv_2d', (f, k, sx, sy), L, np.random.default_rng(0))
  theta += (0.03 * np.random.default_rng(1).standard_normal(theta.size)).astype(np.float32)
  cfg = vo.random_configurations(n, b, np.random.RandomState(2))
  bonds = vo.torus_bonds(sx, sy)
  out = []
  for eng in (VmcEngine(n, b, L, f, ansatz='conv_2d', kernel_size=k, size_x=sx, size_y=sy, seed=2024),
              _engine(adj, L, f, b, 'relu')):
    assert eng.kernel_path() == 6
    eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, -1.0, 1.0)
    logit = eng.amplitude()[0]
    eloc = eng.local_energy()[0]
    eng.mc_steps(2 * n)
    chains = eng.get_configs()
    eng.reset_accumulators()
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    out.append((logit, eloc, chains, eng.get_accumulators(), eng.amplitude()[0]))
    eng.close()
  (l0, e0, c0, a0, m0), (l1, e1, c1, a1, m1) = out
  np.testing.assert_array_equal(l1, l0)
  np.testing.assert_array_equal(e1, e0)
  np.testing.assert_array_equal(c1, c0)
  np.testing.assert_array_equal(m1, m0)
  p = theta.size
  for s in (slice(0, p), slice(p, 2 * p)):
    assert np.abs(a1[s] - a0[s]).max() <= 1e-5 * np.abs(a0[s]).max() + 1e-6
  np.testing.assert_array_equal(a1[2 * p:], a0[2 * p:])


def _check_forward(eng, theta, cfg, adj, f, L, nonlin, b2=13):
  """Amplitudes of the chains (the cached path) and of a second batch of another size against fp64."""
  _logits_close(eng.amplitude()[0], theta, cfg, adj, f, L, nonlin)
  c2 = vo.random_configurations(adj.shape[0], b2, np.random.RandomState(9))
  _logits_close(eng.amplitude(c2)[0], theta, c2, adj, f, L, nonlin)


def _check_local_energy(eng, theta, cfg, adj, bonds, f, L, nonlin, oact, scaled=False):
  """scaled: the bound of tests/test_gpu_conv_general.py::test_general_convolution_random_shapes, which follows the
  logits' rounding where sum |last map| is large."""
  amp = lambda c: go.gnn_psi(theta, c, adj, f, L, -10.0, nonlin, oact)
  rel = 2e-4
  if scaled:
    rel = max(2e-4, 4e-6 * float(np.max(go.gnn_forward(theta, cfg, adj, f, L, nonlin, return_tape='scale')[1])))
  _close(eng.local_energy()[0], vo.local_value(amp, cfg, bonds, -1.0, 1.0, dtype=np.float64), rel)


def _check_sampler_steps(eng, theta, cfg, adj, f, L, nonlin, oact):
  """12 steps against the oracle's sampler on the same Philox streams (chains within 1e-4 of a tie excluded); returns
  the engine's chains."""
  b = cfg.shape[0]
  eng.step_counter = 0
  cur, ok = gsc.oracle_steps(theta, cfg, adj, f, L, nonlin, oact)
  eng.mc_steps(gsc.STEPS)
  got = eng.get_configs()
  np.testing.assert_array_equal(got[ok], cur[ok])
  assert ok.sum() > b // 2 and (got.sum(1) == cfg.sum(1)).all()
  return got


def _check_energy_gradient(eng, theta, got, adj, bonds, f, L, nonlin, oact):
  """EnergyGradient accumulators (training.py:539-558) of the chains `got`."""
  acc = vo.Accumulators(theta.size, np.float64)
  go.energy_gradient_accumulate(acc, theta, got, bonds, -1.0, 1.0, -10.0, adj, f, L, nonlin, oact)
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  res = eng.get_accumulators()
  _acc_close(res, acc, theta.size)
  assert abs(res[2 * theta.size] - acc.e_total) < 2e-4 * max(1, abs(acc.e_total))


def _check_log_overlap(eng, theta, theta_w, got, adj, bonds, f, L, nonlin, oact):
  """LogOverlapITSWO accumulators (training.py:661-695) against a different supervisor."""
  eng.set_params(theta_w, _hip.VMC_OMEGA)
  eng.set_shift(-10.0, _hip.VMC_OMEGA)
  acc = vo.Accumulators(theta.size, np.float64)
  go.log_overlap_accumulate(acc, theta, theta_w, got, bonds, -1.0, 1.0, -10.0, -10.0, 0.05, adj, f, L, nonlin, oact)
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.05)
  res = eng.get_accumulators()
  _acc_close(res, acc, theta.size)
  assert abs(res[2 * theta.size + 2] - acc.r_total) < 2e-4 * max(1, abs(acc.r_total))


@pytest.mark.parametrize('graph,L,f,b,nonlin,oact', CASES, ids=[c[0] for c in CASES])
def test_gnn_fp64_parity(graph, L, f, b, nonlin, oact):
  adj, bonds = GRAPHS[graph]
  n, k = adj.shape
  rng = np.random.default_rng(3)
  theta = go.gnn_init_params(k, f, L, rng, noise=0.03 if f <= 16 else 0.01)
  cfg = vo.random_configurations(n, b, np.random.RandomState(4))
  eng = _engine(adj, L, f, b, nonlin, oact)
  assert eng.kernel_path() == 6 and eng.num_params == theta.size == go.gnn_num_params(k, f, L)
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, -1.0, 1.0)
  _check_forward(eng, theta, cfg, adj, f, L, nonlin)
  _check_local_energy(eng, theta, cfg, adj, bonds, f, L, nonlin, oact)
  got = _check_sampler_steps(eng, theta, cfg, adj, f, L, nonlin, oact)
  _check_energy_gradient(eng, theta, got, adj, bonds, f, L, nonlin, oact)
  theta_w = (theta + 0.02 * rng.standard_normal(theta.size)).astype(np.float32)
  _check_log_overlap(eng, theta, theta_w, got, adj, bonds, f, L, nonlin, oact)
  eng.close()


def _check_sr(adj, bonds):
  """One SR solve on a gnn ctx against the dense fp64 solve on the oracle's per-sample gradients, checked as
  tests/test_gpu_conv_general.py checks the periodic path."""
  n, k = adj.shape
  L, f, b, n_store = 2, 8, 16, 2
  rng = np.random.default_rng(8)
  theta = go.gnn_init_params(k, f, L, rng)
  eng = _engine(adj, L, f, b, 'tanh')
  eng.set_params(theta); eng.set_bonds(bonds, -1.0, 1.0)
  eng.sr_reserve(n_store)
  eng.reset_accumulators()
  cfgs, elocs = [], []
  for j in range(n_store):
    eng.set_configs(vo.random_configurations(n, b, np.random.RandomState(50 + j)))
    eng.mc_steps(2)
    cfgs.append(eng.get_configs())
    eng.accumulate(0)
    elocs.append(eng.local_energy()[0])
  cfg_all = np.concatenate(cfgs, 0)
  e = np.concatenate(elocs, 0).astype(np.float64)
  o = go.gnn_per_sample_grads(theta, cfg_all, adj, f, L, 'tanh')
  s_mat, f_vec = vo.sr_system(o, e)
  v = rng.standard_normal(theta.size).astype(np.float32)
  cancel = np.abs(o).mean(0).max() * np.abs(o @ v.astype(np.float64)).mean()
  ref = s_mat @ v.astype(np.float64)
  got = eng.sr_debug_matvec(v, 0.0)
  assert np.abs(got - ref).max() <= 5e-4 * np.abs(ref).max() + 4e-6 * cancel
  lam = 1e-2
  iters, res = eng.sr_solve(lam, 1e-6, 3000)
  x = eng.sr_get_solution()
  assert res <= 1e-4, (iters, res)
  resid = (s_mat + lam * np.eye(theta.size)) @ x.astype(np.float64) - f_vec
  f_round = 4e-6 * np.abs(o).mean(0).max() * np.abs(e).mean() * np.sqrt(theta.size)
  assert np.linalg.norm(resid) <= 2e-3 * np.linalg.norm(f_vec) + f_round
  oc = o - o.mean(0)
  x_ref = vo.sr_solve(o, e, lam)
  assert np.abs(oc @ x - oc @ x_ref).max() <= 1e-2 * np.abs(oc @ x_ref).max() + 1e-5
  eng.close()


def test_gnn_stochastic_reconfiguration():
  """One SR solve on a gnn ctx (irregular graph: the col2im backward in every CG iteration) against the dense fp64
  solve on the oracle's per-sample gradients, checked as tests/test_gpu_conv_general.py checks the periodic path."""
  _check_sr(*GRAPHS['irregular-12'])


def test_gnn_sharded_chains_match_one_ctx():
  """Two ctxs owning the halves of the chains (chain_offset) draw the same Philox streams as one ctx: the same
  chains, and accumulator sums that add up to the one ctx's."""
  adj, bonds = GRAPHS['triangular-4x4']
  n, k = adj.shape
  L, f, b = 2, 12, 32
  theta = go.gnn_init_params(k, f, L, np.random.default_rng(11))
  cfg = vo.random_configurations(n, b, np.random.RandomState(12))
  one = _engine(adj, L, f, b, 'relu')
  halves = [_engine(adj, L, f, b // 2, 'relu', chain_offset=r * (b // 2)) for r in range(2)]
  for r, eng in enumerate([one] + halves):
    eng.set_params(theta); eng.set_bonds(bonds, -1.0, 1.0)
    eng.set_configs(cfg if r == 0 else cfg[(r - 1) * (b // 2):r * (b // 2)])
    eng.mc_steps(20)
    eng.reset_accumulators()
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  np.testing.assert_array_equal(np.concatenate([h.get_configs() for h in halves]), one.get_configs())
  a = one.get_accumulators()
  s = halves[0].get_accumulators() + halves[1].get_accumulators()
  p = theta.size
  assert np.abs(s[:2 * p] - a[:2 * p]).max() <= 1e-5 * np.abs(a[:2 * p]).max() + 1e-6
  assert abs(s[2 * p] - a[2 * p]) <= 1e-5 * abs(a[2 * p]) + 1e-5 and s[2 * p + 1] == a[2 * p + 1]
  for eng in [one] + halves:
    eng.close()


def test_gnn_run_training_and_energy_evaluation(tmp_path, monkeypatch):
  """run_training --wavefunction_type=gnn on the 5-point graph of the 4 x 4 Heisenberg torus (j_x = -1, exact
  E0 = -11.2285) reaches <= -10.89 within 20 s; run_energy_evaluation reloads it from the same directory (.npz
  checkpoints), and a shorter run's TF bundles (CGS_VMC_CHECKPOINT_FORMAT=tf) reload the same way."""
  import time
  from cgs_vmc_amd import lattice, run_energy_evaluation, run_training, session, wavefunctions
  monkeypatch.setenv('CGS_VMC_INIT_SEED', '7')
  adj_path = str(tmp_path / 'adjacency.txt')
  np.savetxt(adj_path, go.square_5point_adjacency(4, 4), fmt='%d')
  for fmt, epochs in (('npz', 400), ('tf', 40)):
    monkeypatch.setenv('CGS_VMC_CHECKPOINT_FORMAT', fmt)
    session.reset_default_graph(); wavefunctions.reset_name_scope()
    d = str(tmp_path / fmt)
    os.makedirs(d)
    lattice.write_bonds(d, lattice.torus_bonds(4, 4))
    hp = ('batch_size=512,num_conv_layers=2,num_conv_filters=16,nonlinearity=tanh,num_equilibration_sweeps=10,'
          'num_batches_per_epoch=20,learning_rates=[0.003,0.001],learning_rate_stops=[200],'
          'num_evaluation_samples=20,adjacency_list_path=' + adj_path)
    t0 = time.time()
    run_training.main(['--checkpoint_dir', d, '--num_sites', '16', '--heisenberg_jx', '-1.0',
                       '--wavefunction_type', 'gnn', '--optimizer', 'EnergyGradient',
                       '--num_epochs', str(epochs), '--hparams', hp])
    elapsed = time.time() - t0
    energies = [float(x) for x in open(os.path.join(d, 'metrics.txt')).read().split()]
    assert len(energies) == epochs and np.isfinite(energies).all()
    session.reset_default_graph(); wavefunctions.reset_name_scope()
    mean, _ = run_energy_evaluation.main(['--checkpoint_dir', d, '--heisenberg_jx', '-1.0'])
    if fmt == 'npz':
      assert elapsed < 20.0, elapsed
      assert os.path.exists(os.path.join(d, 'model_prior_%d_epochs.npz' % (epochs - 1)))
      assert -11.2285 - 0.1 < mean <= -10.89, (mean, energies[-5:], elapsed)
    else:
      assert not any(f.endswith('.npz') for f in os.listdir(d))
      assert abs(mean - energies[-1]) < 0.6, (mean, energies[-3:])

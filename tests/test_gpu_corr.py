"""GPU: spin correlations (vmc_pair_correlations: csrc/vmc_api_measure.hip + corr.hip; SpinCorrelationEvaluator).

Bounds.  The rows a measurement folds are the local-energy rows of the ansatz type, so the per-pair MEANS are held to the
bounds the types' own local-energy tests apply (tests/test_gpu_engine.py, test_gpu_conv.py, test_gpu_pbdg.py,
test_gpu_edvec.py): dense and convolutional 2e-4 max(1, max|ref|); pbdg rtol 2e-3 with atol 2e-3 mean|ref|; ed_vector
(n_b + 3) 2^-24 (|diag| + sum|terms|) per chain from the vector's own terms.  The fold itself is fp64 over fp32 rows in a
fixed order: against a host fp64 sum of the same rows it is held to B 2^-53 sum|rows|, and to bit equality across pass
splits and repeated calls.
"""
import functools

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from cgs_vmc_amd import lattice
from oracle import vmc_oracle as vo
from tests import corr_oracle as co
from tests import edvec_oracle as eo
from tests import pbdg_oracle as po

pytestmark = pytest.mark.gpu
N, H, B = 16, 32, 40                       # 4 x 4 torus; 40 chains: not a multiple of the 16-chain tiles
PAIRS = lattice.all_pairs(N)               # 120
BONDS = sorted({(min(i, j), max(i, j)) for i, j in vo.torus_bonds(4, 4)})


def _engine(ansatz='fully_connected', n=N, b=B, **kw):
  from cgs_vmc_amd.engine import VmcEngine
  kw.setdefault('seed', 2024)
  if ansatz == 'conv_2d':
    return VmcEngine(n, b, 2, 8, ansatz=ansatz, kernel_size=3, size_x=4, size_y=4, **kw)
  if ansatz == 'pbdg':
    return VmcEngine(n, b, 1, 1, ansatz=ansatz, **kw)
  if ansatz == 'ed_vector':
    top, bot, length = eo.lin_tables(n)
    return VmcEngine(n, b, 1, length, ansatz=ansatz, lin_tables=(top, bot), **kw)
  return VmcEngine(n, b, 1 if ansatz == 'rbm' else 2, H, ansatz=ansatz, **kw)


def _family(ansatz, seed=0):
  """(theta fp32, psi(configs) fp64 oracle)."""
  rng = np.random.default_rng(seed)
  if ansatz == 'fully_connected':
    theta = vo.init_params(N, H, 2, rng)
    return theta, lambda c: vo.fc_psi(theta, c, H, 2, dtype=np.float64)
  if ansatz == 'rbm':
    theta = vo.rbm_init_params(N, H, 1, rng)
    return theta, lambda c: vo.rbm_psi(theta, c, H, 1, dtype=np.float64)
  if ansatz == 'conv_2d':
    geom = (8, 3, 4, 4)
    theta = vo.conv_init_params('conv_2d', geom, 2, rng)
    theta = theta + (0.03 * rng.standard_normal(theta.size)).astype(np.float32)
    return theta, lambda c: vo.ANSATZ['conv_2d'][0](theta, c, geom, 2, dtype=np.float64)
  if ansatz == 'pbdg':
    lim = np.sqrt(3.0 / N)
    theta = rng.uniform(-lim, lim, N * N).astype(np.float32)
    return theta, lambda c: po.psi(theta, c, -10.0)
  top, bot, length = eo.lin_tables(N)
  theta = rng.standard_normal(length).astype(np.float32)
  return theta, lambda c: eo.amplitude(theta, c, top, bot)


@functools.lru_cache(maxsize=None)
def _exact_4x4():
  """(E0, vector in Lin order fp64, top, bot) of the 4 x 4 Heisenberg torus at jx = jz = 1: a total-spin singlet."""
  return eo.vector_from_ed(N, BONDS, 1.0, 1.0)


def _cfg(seed, b=B, n=N):
  return vo.random_configurations(n, b, np.random.RandomState(seed))


def test_fold_equals_the_host_sum_of_the_librarys_own_rows():
  theta, _ = _family('fully_connected')
  cfg = _cfg(1)
  eng = _engine()
  eng.set_params(theta); eng.set_configs(cfg)
  zz, ex = eng.pair_correlations(PAIRS)              # (no Hamiltonian set: the measurement needs none)
  ref_zz = (cfg[:, PAIRS[:, 0]].astype(np.int64) * cfg[:, PAIRS[:, 1]].astype(np.int64)).sum(0)
  np.testing.assert_array_equal(zz, ref_zz.astype(np.float64))
  worst = 0.0
  for k in range(0, 120, 10):                        # a dozen pairs, one single-bond Hamiltonian each: one row per chain
    eng.set_bonds([tuple(PAIRS[k])], 2.0, 0.0)
    diag, rows = eng.local_energy_terms()
    assert (diag == 0).all()
    anti = cfg[:, PAIRS[k, 0]] * cfg[:, PAIRS[k, 1]] < 0
    assert (rows[~anti] == 0).all() and anti.any()
    host = 0.0
    for v in rows.astype(np.float64):                # ascending chain order, fp64: the fold's own order
      host += v
    bound = B * 2.0 ** -53 * np.abs(rows.astype(np.float64)).sum()
    worst = max(worst, abs(ex[k] - host) / bound)
    print('pair %s: fold %.17g host %.17g |diff| %.3g (bound %.3g)' % (tuple(PAIRS[k]), ex[k], host, abs(ex[k] - host), bound))
    assert abs(ex[k] - host) <= bound, (k, ex[k], host)
  print('fold vs host sum of the rows: worst |diff| / bound = %.3g' % worst)
  # the Hamiltonian set by vmc_set_bonds is still the single bond of the last iteration after another measurement
  d0, r0 = eng.local_energy_terms()
  eng.pair_correlations(PAIRS[:7])
  d1, r1 = eng.local_energy_terms()
  np.testing.assert_array_equal(r0, r1); np.testing.assert_array_equal(d0, d1)
  eng.close()


def _mean_bound(ansatz, ref, theta, cfg):
  if ansatz == 'pbdg':
    return 2e-3 * np.abs(ref) + 2e-3 * np.abs(ref).mean()
  if ansatz == 'ed_vector':
    top, bot, _ = eo.lin_tables(N)
    sz, ratio = co.pair_terms(lambda c: eo.amplitude(theta, c, top, bot), cfg, PAIRS)
    # per chain and pair: one term (n_b = 1 where antiparallel), diag = s_i s_j / 4, term = ratio / 2; the mean over chains
    return (((ratio != 0) + 3) * 2.0 ** -24 * (0.25 * np.abs(sz) + 0.5 * np.abs(ratio))).mean(0)
  return np.full(len(ref), 2e-4 * max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize('ansatz', ['fully_connected', 'rbm', 'conv_2d', 'pbdg', 'ed_vector'])
def test_pair_means_match_the_independent_oracle(ansatz):
  theta, psi = _family(ansatz)
  cfg = _cfg(2)
  assert (cfg.sum(1) == 0).all()
  eng = _engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg)
  zz, ex = eng.pair_correlations(PAIRS)
  ref_zz, ref_ex = co.pair_sums(psi, cfg, PAIRS)
  np.testing.assert_array_equal(zz, ref_zz)
  _, ref_exch, ref_ss = co.pair_means(psi, cfg, PAIRS)
  got_ss = (0.25 * zz + 0.5 * ex) / B
  for name, got, ref in (('exchange', 0.5 * ex / B, ref_exch), ('ss', got_ss, ref_ss)):
    bound = _mean_bound(ansatz, ref, theta, cfg)
    err = np.abs(got - ref)
    k = (err / bound).argmax()
    print('%s %s: max error %.3g, worst error / bound %.3g (error %.3g, bound %.3g)' % (ansatz, name, err.max(), err[k] / bound[k], err[k], bound[k]))
    assert (err <= bound).all(), (name, err[k], bound[k])
  # the supervisor's parameter set measures through the same entry
  eng.set_params(theta, _hip.VMC_OMEGA)
  zz_w, ex_w = eng.pair_correlations(PAIRS, which=_hip.VMC_OMEGA)
  np.testing.assert_array_equal(zz_w, zz); np.testing.assert_array_equal(ex_w, ex)
  eng.close()


def test_pass_splits_and_repeats_are_bit_identical_on_276_pairs():
  """24-site chain, all 276 pairs: past the 256-bond prefetch groups of the list kernels, no multiple of 64."""
  n = 24
  pairs = lattice.all_pairs(n)
  assert len(pairs) == 276
  theta = vo.init_params(n, H, 2, np.random.default_rng(3))
  cfg = _cfg(4, n=n)
  eng = _engine(n=n)
  eng.set_params(theta); eng.set_configs(cfg)
  base = eng.pair_correlations(pairs)
  ref_zz, ref_ex = co.pair_sums(lambda c: vo.fc_psi(theta, c, H, 2, dtype=np.float64), cfg, pairs)
  np.testing.assert_array_equal(base[0], ref_zz)
  assert np.abs(0.5 * (base[1] - ref_ex) / B).max() <= 2e-4 * max(1.0, np.abs(0.5 * ref_ex / B).max())
  for per in (0, 1, 7, 64, 276):
    for _ in range(2):
      zz, ex = eng.pair_correlations(pairs, pairs_per_pass=per)
      np.testing.assert_array_equal(zz, base[0], err_msg='pairs_per_pass=%d' % per)
      np.testing.assert_array_equal(ex, base[1], err_msg='pairs_per_pass=%d' % per)
  # ... nor on which other pairs are in the list, or where
  pick = np.random.default_rng(5).permutation(276)[:50]
  zz, ex = eng.pair_correlations(pairs[pick], pairs_per_pass=9)
  np.testing.assert_array_equal(zz, base[0][pick]); np.testing.assert_array_equal(ex, base[1][pick])
  eng.close()


def _state(eng):
  return (eng.local_energy()[0], eng.get_configs(), eng.step_counter, eng.get_accumulators())


def test_a_measurement_moves_nothing_else():
  theta, _ = _family('fully_connected')
  eng = _engine()
  eng.set_params(theta); eng.set_configs(_cfg(6)); eng.set_bonds(BONDS, 1.0, 1.0)
  eng.mc_steps(3 * N)
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  before = _state(eng)
  eng.pair_correlations(PAIRS); eng.pair_correlations(PAIRS, pairs_per_pass=7)
  after = _state(eng)
  for x, y in zip(before, after):
    np.testing.assert_array_equal(x, y)
  eng.mc_steps(N)                                    # straight from the sampler's caches and census into a measurement
  eloc = eng.local_energy()[0]
  eng.mc_steps(N); chains = eng.get_configs()
  eng.close()
  eng = _engine()
  eng.set_params(theta); eng.set_configs(_cfg(6)); eng.set_bonds(BONDS, 1.0, 1.0)
  eng.mc_steps(3 * N)
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  eng.mc_steps(N)
  eng.pair_correlations(PAIRS)
  np.testing.assert_array_equal(eng.local_energy()[0], eloc)
  eng.mc_steps(N)
  np.testing.assert_array_equal(eng.get_configs(), chains)
  eng.close()
  # two training epochs with and without a measurement between them: the same parameters
  params = []
  for measure in (False, True):
    eng = _engine(b=64, seed=77)
    eng.set_params(theta); eng.set_configs(_cfg(7, b=64)); eng.set_bonds(BONDS, 1.0, 1.0)
    for epoch in range(2):
      eng.epoch_energy_gradient(2 * N, 3, N, 1e10)
      eng.apply_adam(_hip.VMC_MODE_ENERGY_GRADIENT, 1e-2)
      if measure and epoch == 0:
        eng.pair_correlations(PAIRS, pairs_per_pass=50)
    params.append((eng.get_params(), eng.get_configs(), eng.step_counter))
    eng.close()
  for x, y in zip(*params):
    np.testing.assert_array_equal(x, y)


def _singlet_chains(vec, top, bot, b, seed):
  """b Sz = 0 configurations with |psi| >= 1e-5 (the cut of the ed_vector pin in tests/test_gpu_edvec.py)."""
  cfg = _cfg(seed, b=4 * b)
  keep = np.abs(eo.amplitude(vec, cfg, top, bot)) >= 1e-5
  assert keep.sum() >= b
  return np.ascontiguousarray(cfg[keep][:b])


def test_exact_singlet_total_spin_is_zero_on_every_set_of_chains():
  """S^2 psi = 0 configuration by configuration: sum_{i<j} (zz / 4 + ex / 2) / B = -3 N / 8 with no Monte-Carlo error."""
  e0, vec, top, bot = _exact_4x4()
  cfg = _singlet_chains(vec, top, bot, B, 8)
  psi64 = lambda c: eo.amplitude(vec, c, top, bot)
  sz, ratio = co.pair_terms(psi64, cfg, PAIRS)
  per_chain = (0.25 * sz + 0.5 * ratio).sum(1)
  oracle_dev = np.abs(per_chain + 3 * N / 8.0).max()
  print('fp64 eigenvector: max |sum_{i<j} local + 3N/8| per chain = %.3g' % oracle_dev)
  vec32 = vec.astype(np.float32)
  sz32, ratio32 = co.pair_terms(lambda c: eo.amplitude(vec32, c, top, bot), cfg, PAIRS)
  bound = (((ratio32 != 0).sum(1) + 3) * 2.0 ** -24 * (np.abs(0.25 * sz32.sum(1)) + np.abs(0.5 * ratio32).sum(1))).mean()
  assert oracle_dev <= 1e-3 * bound, (oracle_dev, bound)         # the eigenvector itself is a singlet far inside the bound
  eng = _engine('ed_vector')
  eng.set_params(vec32); eng.set_configs(cfg)
  zz, ex = eng.pair_correlations(PAIRS)
  total = ((0.25 * zz + 0.5 * ex) / B).sum()
  print('sum_{i<j} <S_i.S_j> over %d chains = %.9f (exact %.3f): deviation %.3g, bound %.3g' % (B, total, -3 * N / 8.0, abs(total + 3 * N / 8.0), bound))
  assert abs(total + 3 * N / 8.0) <= bound
  eng.close()


def test_evaluator_reproduces_the_exact_correlations_within_five_sigma(monkeypatch, tmp_path):
  from cgs_vmc_amd import evaluation, run_correlation_evaluation as rc, session, wavefunctions
  from tools import make_ed_vector as mk
  e0, vec, top, bot = _exact_4x4()
  exact = co.expectation(lambda c: eo.amplitude(vec, c, top, bot), eo.sz0_configurations(N), PAIRS)
  assert abs(exact.sum() + 3 * N / 8.0) < 1e-9
  index = {(int(i), int(j)): k for k, (i, j) in enumerate(PAIRS)}
  nn = np.array([index[b] for b in BONDS])
  assert abs(exact[nn].sum() - e0) < 1e-9
  monkeypatch.setenv('CGS_VMC_SEED', '20241018')
  monkeypatch.setenv('CGS_VMC_CONFIG_SEED', '5')
  d = str(tmp_path / 'ed')
  assert abs(mk.main([d, '--lattice', 'square', '--size', '4', '4']) - e0) < 1e-9
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  # The standard error of the evaluator is the conventional one, std / sqrt(n) of the batch means: it is an error bar only
  # for decorrelated samples.  A sweep is N = 16 exchange proposals per chain, about half of them accepted, and moves two
  # spins at most each: the default of ONE sweep between samples leaves consecutive batch means correlated (measured on an
  # MI355X with this seed: worst pair 5.13 of its reported errors, three more pairs above 4).  Ten sweeps (160 proposals per
  # chain on 16 sites) are taken between samples here.
  result, written = rc.main(['--checkpoint_dir', d, '--hparams',
                             'batch_size=1024,num_evaluation_samples=20,num_monte_carlo_sweeps=10,size_x=4,size_y=4'])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  np.testing.assert_array_equal(result['pairs'], PAIRS)
  dev = np.abs(result['ss'] - exact) / result['ss_err']
  print('evaluator, 1024 chains x 20 samples: worst |<S_i.S_j> - exact| / err = %.2f (pair %s); mean err %.3g'
        % (dev.max(), tuple(PAIRS[dev.argmax()]), result['ss_err'].mean()))
  assert (result['ss_err'] > 0).all() and (dev <= 5.0).all(), (dev.max(), PAIRS[dev.argmax()])
  # the nearest-neighbour sum times J is the energy
  e_samples = result['samples'][:, 2][:, nn].sum(1)
  e_mean, e_err = e_samples.mean(), e_samples.std(ddof=1) / np.sqrt(len(e_samples))
  print('nearest-neighbour sum %.6f +/- %.2g (E0 = %.6f)' % (e_mean, e_err, e0))
  # (the energy of an eigenstate has no Monte-Carlo spread: what is left is the fp32 rounding of the vector, under the
  # ed_vector local-energy rule with n_b <= 32 bonds, |diag| <= 32 / 4 and sum|terms| = |sum terms| -- Marshall's sign rule
  # makes every nearest-neighbour term of this state negative)
  rounding = (len(BONDS) + 3) * 2.0 ** -24 * (0.25 * len(BONDS) + abs(result['exchange'][nn].sum()))
  assert abs(e_mean - e0) <= 5.0 * e_err + rounding, (e_mean - e0, e_err, rounding)
  # the two files of the command-line driver
  assert [p.rsplit('/', 1)[1] for p in written] == ['correlations.txt', 'structure_factor.txt']
  rows = np.loadtxt(written[0])
  assert rows.shape == (120, 6)
  np.testing.assert_allclose(rows[:, 4], result['ss'], rtol=1e-9)
  sq = np.loadtxt(written[1])
  assert sq.shape == (16, 3)
  np.testing.assert_allclose(sq[:, 2], lattice.structure_factor(result['ss'], PAIRS, lattice.torus_coords(4, 4), sq[:, :2]), rtol=1e-8)
  assert sq[:, 2].argmax() == 10 and np.allclose(sq[10, :2], np.pi)          # the peak sits at (pi, pi)


def test_refusals():
  from cgs_vmc_amd.engine import VmcEngine
  theta, _ = _family('fully_connected')
  eng = _engine()
  eng.set_configs(_cfg(9))
  with pytest.raises(_hip.HipLibraryError, match='parameters not set'):
    eng.pair_correlations(PAIRS)
  eng.set_params(theta)
  for bad in ([(3, 3)], [(0, N)], [(-1, 2)], [(0, 1), (5, 5)]):
    with pytest.raises(ValueError, match='pair'):
      eng.pair_correlations(bad)
  with pytest.raises(ValueError):
    eng.pair_correlations(PAIRS, which=2)
  with pytest.raises(ValueError):
    eng.pair_correlations(PAIRS, pairs_per_pass=-1)
  with pytest.raises(ValueError):
    eng.pair_correlations(np.zeros((0, 2), np.int32))
  zz, ex = eng.pair_correlations([(1, 0)])             # either orientation is the same pair
  zz2, ex2 = eng.pair_correlations([(0, 1)])
  assert zz == zz2 and ex == ex2
  eng.close()
  spec = dict(ansatz='fully_connected', num_layers=1, layer_size=H, nonlinearity='relu', output_activation='exp')
  prod = VmcEngine(N, B, 0, 0, ansatz='prod', children=[spec, dict(spec, ansatz='rbm')], seed=2024)
  with pytest.raises(NotImplementedError, match='product ctx'):
    prod.pair_correlations(PAIRS)
  with pytest.raises(_hip.ComposedFactorError):
    prod.children[0].pair_correlations(PAIRS)
  prod.close()

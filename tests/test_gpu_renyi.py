"""GPU: the replica swap estimator of the second Renyi entropy (vmc_renyi2_swap: csrc/vmc_api_measure.hip + renyi.hip;
RenyiEntropyEvaluator; run_entanglement_evaluation) against the fp64 oracle tests/renyi_oracle.py.

Bound.  A pair's term is exp of the sum of four fp32 logs ln|psi| (two swapped rows minus the two chains), formed in fp64.
With eps_r the bound the family's own amplitude / logit parity test applies to ln|psi| of row r (the constants below, each
next to the file it is taken from), the term is within |term_ref| (exp(eps_x~ + eps_y~ + eps_x + eps_y) - 1) of the
oracle's, and the fp64 fold of P = B / 2 terms in a fixed order adds P 2^-53 sum |term_ref|:
  |swap_sum - ref| <= sum_c |term_ref_c| (exp(sum of the four eps) - 1) + (B / 2) 2^-53 sum_c |term_ref_c|
(with one eps for all rows this is the sum_c |term_ref| (exp(4 eps) - 1) form).  match_count is an integer: bit-equal.
"""
import functools

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from cgs_vmc_amd import lattice
from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo
from tests import gnn_oracle as go
from tests import nnb_oracle as no
from tests import pbdg_oracle as po
from tests import renyi_oracle as ro

pytestmark = pytest.mark.gpu
N, H, B = 16, 32, 40                       # 4 x 4 torus; 40 chains = 20 pairs: no multiple of the 8- or 16-chain tiles
HALF = B // 2
EPS32 = np.finfo(np.float32).eps
BONDS = sorted({(min(i, j), max(i, j)) for i, j in vo.torus_bonds(4, 4)})
SCATTERED = [1, 4, 6, 11, 14]
# blocks l = 1 .. 8, one scattered region, the empty region, the full set
REGIONS = lattice.block_regions(N) + [SCATTERED, [], list(range(N))]
MASKS = ro.masks(REGIONS, N)
FAMILIES = ['fully_connected', 'rbm', 'conv_2d', 'gnn', 'pbdg', 'fully_connected_nnb', 'ed_vector']
GNN_ADJ = go.triangular_adjacency(4, 4)
CONV_GEOM = (8, 3, 4, 4)


def _engine(ansatz='fully_connected', n=N, b=B, **kw):
  from cgs_vmc_amd.engine import VmcEngine
  kw.setdefault('seed', 2024)
  if ansatz == 'conv_2d':
    return VmcEngine(n, b, 2, 8, ansatz=ansatz, kernel_size=3, size_x=4, size_y=4, **kw)
  if ansatz == 'gnn':
    return VmcEngine(n, b, 2, 8, ansatz=ansatz, adjacency=GNN_ADJ, **kw)
  if ansatz == 'pbdg':
    return VmcEngine(n, b, 1, 1, ansatz=ansatz, **kw)
  if ansatz == 'ed_vector':
    top, bot, length = eo.lin_tables(n)
    return VmcEngine(n, b, 1, length, ansatz=ansatz, lin_tables=(top, bot), **kw)
  return VmcEngine(n, b, 1 if ansatz == 'rbm' else 2, H, ansatz=ansatz, **kw)


def _family(ansatz, seed=0):
  """(theta fp32, psi(configs) fp64 oracle, eps(configs) -> the per-row bound on ln|psi| of the family's parity test)."""
  rng = np.random.default_rng(seed)
  if ansatz == 'fully_connected':
    theta = vo.init_params(N, H, 2, rng)
    # tests/test_gpu_engine.py (test_amplitude_matches_oracle): |dlogit| <= 2e-5 max(1, |logit|)
    eps = lambda c: 2e-5 * np.maximum(1.0, np.abs(vo.fc_logit(theta, c, H, 2, dtype=np.float64)))
    return theta, (lambda c: vo.fc_psi(theta, c, H, 2, dtype=np.float64)), eps
  if ansatz == 'rbm':
    theta = vo.rbm_init_params(N, H, 1, rng)
    # tests/test_gpu_rbm.py (test_rbm_amplitude_and_local_energy): |dlogit| <= 2e-5 max(1, |logit|)
    eps = lambda c: 2e-5 * np.maximum(1.0, np.abs(vo.rbm_logit(theta, c, H, 1, dtype=np.float64)))
    return theta, (lambda c: vo.rbm_psi(theta, c, H, 1, dtype=np.float64)), eps
  if ansatz == 'conv_2d':
    theta = vo.conv_init_params('conv_2d', CONV_GEOM, 2, rng)
    theta = theta + (0.03 * rng.standard_normal(theta.size)).astype(np.float32)
    # tests/test_gpu_conv.py (_logits_close): |dlogit| <= 1e-6 sum |entries of the last map| + 2e-5
    eps = lambda c: 1e-6 * vo.conv_forward(theta, c, 'conv_2d', CONV_GEOM, 2, 'relu', np.float64, return_tape='scale')[1] + 2e-5
    return theta, (lambda c: vo.ANSATZ['conv_2d'][0](theta, c, CONV_GEOM, 2, dtype=np.float64)), eps
  if ansatz == 'gnn':
    theta = go.gnn_init_params(GNN_ADJ.shape[1], 8, 2, rng)
    # tests/test_gpu_gnn.py (_logits_close): |dlogit| <= 1e-6 sum |entries of the last map| + 2e-5
    eps = lambda c: 1e-6 * go.gnn_forward(theta, c, GNN_ADJ, 8, 2, 'relu', return_tape='scale')[1] + 2e-5
    return theta, (lambda c: go.gnn_psi(theta, c, GNN_ADJ, 8, 2)), eps
  if ansatz == 'pbdg':
    lim = np.sqrt(3.0 / N)
    theta = rng.uniform(-lim, lim, N * N).astype(np.float32)
    # tests/test_gpu_pbdg.py (_amplitudes_close): |dlogit| <= 64 (N / 2) eps32 kappa(M) per row
    eps = lambda c: 64 * (N // 2) * EPS32 * po.condition_numbers(theta, c)
    return theta, (lambda c: po.psi(theta, c, -10.0)), eps
  if ansatz == 'fully_connected_nnb':
    theta = no.default_theta(N, 2, H, 1)
    # tests/test_gpu_nnb.py (test_nnb_amplitudes_match_the_fp64_oracle): |dlogit| <= 64 (N / 2) eps32 kappa(M) per row
    eps = lambda c: 64 * (N // 2) * EPS32 * no.condition_numbers(theta, c, 2, H)
    return theta, (lambda c: no.psi(theta, c, 2, H)), eps
  top, bot, length = eo.lin_tables(N)
  theta = rng.standard_normal(length).astype(np.float32)
  theta[::7] = 0.0                                     # zero entries: their pairs give exactly 0, never NaN
  return theta, (lambda c: eo.amplitude(theta.astype(np.float64), c, top, bot)), _edvec_eps(theta, top, bot)


def _edvec_eps(vec32, top, bot):
  """tests/test_gpu_edvec.py (_check_amplitudes): ln|psi| within one fp32 spacing of its own magnitude (rows with
  psi = 0 carry no logarithm: their terms are 0 on both sides)."""
  def eps(c):
    a = np.abs(eo.amplitude(vec32.astype(np.float64), c, top, bot))
    out = np.zeros(len(a))
    nz = a != 0
    out[nz] = np.spacing(np.abs(np.log(a[nz])).astype(np.float32)).astype(np.float64)
    return out
  return eps


def _cfg(seed, b=B, n=N):
  return vo.random_configurations(n, b, np.random.RandomState(seed))


def _reference(psi, eps, cfg, masks):
  """(swap_sum, match_count, bound) [n_regions] from the oracle."""
  cfg = np.asarray(cfg, np.float32)
  half = len(cfg) // 2
  x, y = cfg[:half], cfg[half:]
  terms, match = ro.pair_terms(psi, cfg, masks)
  sums, counts = ro.swap_sums(psi, cfg, masks)
  e_own = eps(x) + eps(y)
  bound = np.zeros(len(masks))
  for k, m in enumerate(np.asarray(masks, bool)):
    xs, ys = x.copy(), y.copy()
    xs[:, m] = y[:, m]; ys[:, m] = x[:, m]
    e4 = e_own.copy()
    hit = match[k]
    if hit.any():
      e4[hit] += eps(xs[hit]) + eps(ys[hit])
    a = np.abs(terms[k])
    bound[k] = (a * np.expm1(e4)).sum() + half * 2.0 ** -53 * a.sum()
  return sums, counts, bound


def _check(tag, got, ref, bound):
  err = np.abs(got - ref)
  with np.errstate(divide='ignore', invalid='ignore'):
    rel = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
  k = int(np.argmax(rel))
  print('%s: worst error / bound %.3g (region %d: error %.3g, bound %.3g, value %.9g)' % (tag, rel[k], k, err[k], bound[k], ref[k]))
  assert (err <= bound).all(), (tag, k, err[k], bound[k])


@pytest.mark.parametrize('ansatz', FAMILIES)
def test_swap_sums_match_the_fp64_oracle(ansatz):
  theta, psi, eps = _family(ansatz)
  cfg = _cfg(2)
  assert (cfg.sum(1) == 0).all()
  eng = _engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg)
  swap, match = eng.renyi2_swap(REGIONS)
  ref_swap, ref_match, bound = _reference(psi, eps, cfg, MASKS)
  np.testing.assert_array_equal(match, ref_match)
  assert np.isfinite(swap).all()
  _check(ansatz, swap, ref_swap, bound)
  assert 0 < ref_match[:8].min() and ref_match[:8].max() < HALF       # the blocks see matching and non-matching pairs
  # the empty region and the full set: every pair matches, every term is 1 (0 where a chain's own amplitude vanishes)
  alive = float(((psi(cfg[:HALF]) != 0) & (psi(cfg[HALF:]) != 0)).sum())
  for k in (-2, -1):
    assert match[k] == HALF
    assert abs(swap[k] - alive) <= bound[k], (k, swap[k], alive, bound[k])
  if ansatz != 'ed_vector':
    assert alive == HALF
  # the 0 / 1 array form of the regions is the same call
  swap_m, match_m = eng.renyi2_swap(MASKS.astype(np.uint8))
  np.testing.assert_array_equal(swap_m, swap); np.testing.assert_array_equal(match_m, match)
  # the supervisor's parameter set measures through the same entry
  eng.set_params(theta, _hip.VMC_OMEGA)
  swap_w, match_w = eng.renyi2_swap(REGIONS, which=_hip.VMC_OMEGA)
  np.testing.assert_array_equal(swap_w, swap); np.testing.assert_array_equal(match_w, match)
  eng.close()


@pytest.mark.parametrize('ansatz', ['fully_connected', 'pbdg', 'ed_vector'])
def test_a_region_and_its_complement_agree(ansatz):
  """The two swapped rows just trade places: equal match counts, swap sums within the bound of either side."""
  theta, psi, eps = _family(ansatz)
  cfg = _cfg(3)
  eng = _engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg)
  masks = MASKS[:9]
  swap, match = eng.renyi2_swap(masks.astype(np.uint8))
  swap_c, match_c = eng.renyi2_swap((~masks).astype(np.uint8))
  np.testing.assert_array_equal(match, match_c)
  _, _, bound = _reference(psi, eps, cfg, masks)
  _, _, bound_c = _reference(psi, eps, cfg, ~masks)
  err = np.abs(swap - swap_c)
  print('%s: region vs complement: max |diff| %.3g, worst diff / bound %.3g' % (ansatz, err.max(), (err / (bound + bound_c)).max()))
  assert (err <= bound + bound_c).all()
  eng.close()


def test_a_product_vector_has_purity_one_on_every_set_of_chains():
  """psi(x) = a(x_A) b(x_rest) with random positive factors: every matching pair's term is 1, so swap_sum = match_count
  with no Monte-Carlo error -- on A, on its complement, and for any chains."""
  rng = np.random.default_rng(11)
  top, bot, length = eo.lin_tables(N)
  in_a = np.zeros(N, bool); in_a[SCATTERED] = True
  basis = eo.sz0_configurations(N)
  bits = (basis > 0).astype(np.int64)
  ka = bits[:, in_a] @ (1 << np.arange(int(in_a.sum())))
  kb = bits[:, ~in_a] @ (1 << np.arange(int((~in_a).sum())))
  # factors in [0.5, 1.5) with 12-bit mantissas: their products are exact in fp32, the stored vector IS a product
  fa = rng.integers(1024, 3072, 1 << int(in_a.sum())) / 2048.0
  fb = rng.integers(1024, 3072, 1 << int((~in_a).sum())) / 2048.0
  vec = np.zeros(length, np.float64)
  vec[eo.index(basis, top, bot)] = fa[ka] * fb[kb]
  vec32 = vec.astype(np.float32)
  assert (vec32.astype(np.float64) == vec).all()
  eps = _edvec_eps(vec32, top, bot)
  masks = np.stack([in_a, ~in_a])
  eng = _engine('ed_vector')
  eng.set_params(vec32)
  for seed in (4, 5):
    cfg = _cfg(seed)
    eng.set_configs(cfg)
    swap, match = eng.renyi2_swap(masks.astype(np.uint8))
    ref_swap, ref_match, bound = _reference(lambda c: eo.amplitude(vec, c, top, bot), eps, cfg, masks)
    np.testing.assert_array_equal(match, ref_match)
    np.testing.assert_allclose(ref_swap, ref_match, rtol=1e-14)
    assert 0 < match[0] < HALF
    err = np.abs(swap - match)
    print('product vector, chains %d: |swap_sum - match_count| %s (bound %s)' % (seed, err, bound))
    assert (err <= bound).all()
  eng.close()


def test_pass_splits_and_repeats_are_bit_identical_on_70_regions():
  """70 regions: more than one 64-thread fold block, no multiple of 64."""
  rng = np.random.default_rng(6)
  masks = np.unique(rng.integers(0, 2, (200, N)).astype(np.uint8), axis=0)[:70]
  assert masks.shape == (70, N)
  theta, psi, eps = _family('fully_connected')
  cfg = _cfg(7)
  eng = _engine()
  eng.set_params(theta); eng.set_configs(cfg)
  base = eng.renyi2_swap(masks)
  ref_swap, ref_match, bound = _reference(psi, eps, cfg, masks.astype(bool))
  np.testing.assert_array_equal(base[1], ref_match)
  _check('70 regions', base[0], ref_swap, bound)
  for per in (0, 1, 3):
    for _ in range(2):
      swap, match = eng.renyi2_swap(masks, regions_per_pass=per)
      np.testing.assert_array_equal(swap, base[0], err_msg='regions_per_pass=%d' % per)
      np.testing.assert_array_equal(match, base[1], err_msg='regions_per_pass=%d' % per)
  # ... nor on which other regions are in the list, or where
  pick = rng.permutation(70)[:25]
  swap, match = eng.renyi2_swap(masks[pick], regions_per_pass=4)
  np.testing.assert_array_equal(swap, base[0][pick]); np.testing.assert_array_equal(match, base[1][pick])
  eng.close()


def _state(eng):
  return (eng.local_energy()[0], eng.get_configs(), eng.step_counter, eng.get_accumulators())


def test_a_measurement_moves_nothing_else():
  theta, _, _ = _family('fully_connected')
  eng = _engine()
  eng.set_params(theta); eng.set_configs(_cfg(6)); eng.set_bonds(BONDS, 1.0, 1.0)
  eng.mc_steps(3 * N)
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  before = _state(eng)
  terms = eng.local_energy_terms()
  eng.renyi2_swap(REGIONS); eng.renyi2_swap(REGIONS, regions_per_pass=3)
  after = _state(eng)
  for x, y in zip(before, after):
    np.testing.assert_array_equal(x, y)
  for x, y in zip(terms, eng.local_energy_terms()):    # the Hamiltonian's bond set answers as before
    np.testing.assert_array_equal(x, y)
  eng.mc_steps(N)                                      # straight from the sampler's caches into a measurement
  eloc = eng.local_energy()[0]
  eng.mc_steps(N); chains = eng.get_configs()
  eng.close()
  eng = _engine()
  eng.set_params(theta); eng.set_configs(_cfg(6)); eng.set_bonds(BONDS, 1.0, 1.0)
  eng.mc_steps(3 * N)
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  eng.mc_steps(N)
  eng.renyi2_swap(REGIONS)
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
        eng.renyi2_swap(REGIONS, regions_per_pass=5)
    params.append((eng.get_params(), eng.get_configs(), eng.step_counter))
    eng.close()
  for x, y in zip(*params):
    np.testing.assert_array_equal(x, y)


@functools.lru_cache(maxsize=None)
def _exact_chain12():
  n = 12
  e0, vec, top, bot = eo.vector_from_ed(n, lattice.chain_bonds(n), 1.0, 1.0)
  psi = lambda c: eo.amplitude(vec, c, top, bot)
  basis = eo.sz0_configurations(n)
  return e0, np.array([ro.exact_purity(psi, basis, m) for m in ro.masks(lattice.block_regions(n), n)])


def test_evaluator_reproduces_the_exact_purities_within_five_sigma(monkeypatch, tmp_path):
  """The 12-site Heisenberg chain's exact ground state (tools/make_ed_vector.py), blocks l = 1 .. 6.

  Chosen values: batch_size = 1024 (512 replica pairs), num_evaluation_samples = 20, num_monte_carlo_sweeps = 10.  From the
  oracle on the CPU (200,000 independent pairs drawn from |psi|^2, all six blocks): the standard deviation of one pair's
  term is at most 1.55 of the purity (block l = 5; 1.46 for the largest block l = 6, purity 0.427), so 20 x 512 pairs give
  a relative purity_err of about 1.55 / sqrt(10240) = 1.5 % -- below the 5 % asked for with room for the residual
  correlation of consecutive samples (ten sweeps = 120 exchange proposals per chain on 12 sites apart, as in
  tests/test_gpu_corr.py)."""
  from cgs_vmc_amd import run_entanglement_evaluation as re_, session, wavefunctions
  from tools import make_ed_vector as mk
  n = 12
  e0, exact = _exact_chain12()
  monkeypatch.setenv('CGS_VMC_SEED', '20241018')
  monkeypatch.setenv('CGS_VMC_CONFIG_SEED', '5')
  d = str(tmp_path / 'ed')
  assert abs(mk.main([d, '--lattice', 'chain', '--size', str(n)]) - e0) < 1e-9
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  result, written = re_.main(['--checkpoint_dir', d, '--hparams',
                              'batch_size=1024,num_evaluation_samples=20,num_monte_carlo_sweeps=10'])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  np.testing.assert_array_equal(result['regions'], ro.masks(lattice.block_regions(n), n))
  dev = np.abs(result['purity'] - exact) / result['purity_err']
  rel = result['purity_err'] / result['purity']
  for l in range(6):
    print('block l = %d: purity %.5f +/- %.5f (exact %.5f, %.2f sigma), S2 %.4f +/- %.4f, match fraction %.3f'
          % (l + 1, result['purity'][l], result['purity_err'][l], exact[l], dev[l], result['s2'][l], result['s2_err'][l],
             result['match_fraction'][l]))
  assert rel[-1] < 0.05, rel
  assert (result['purity_err'] > 0).all() and (dev <= 5.0).all(), dev
  np.testing.assert_allclose(result['s2'], -np.log(result['purity']), rtol=1e-14)
  np.testing.assert_allclose(result['s2_err'], result['purity_err'] / result['purity'], rtol=1e-14)
  assert result['samples'].shape == (20, 6)
  # entanglement.txt: one well-formed line per region
  assert [p.rsplit('/', 1)[1] for p in written] == ['entanglement.txt']
  rows = np.loadtxt(written[0])
  assert rows.shape == (6, 6) and np.isfinite(rows).all()
  np.testing.assert_array_equal(rows[:, 0], np.arange(1, 7))
  np.testing.assert_allclose(rows[:, 1], result['purity'], rtol=1e-9)
  np.testing.assert_allclose(rows[:, 3], result['s2'], rtol=1e-9)
  np.testing.assert_allclose(rows[:, 5], result['match_fraction'], rtol=1e-5)


def test_refusals():
  from cgs_vmc_amd.engine import VmcEngine
  theta, _, _ = _family('fully_connected')
  eng = _engine()
  eng.set_configs(_cfg(9))
  with pytest.raises(_hip.HipLibraryError, match='parameters not set'):
    eng.renyi2_swap(REGIONS)
  eng.set_params(theta)
  with pytest.raises(ValueError):
    eng.renyi2_swap(np.zeros((3, N + 1), np.uint8))          # a mask of the wrong shape
  with pytest.raises(ValueError):
    eng.renyi2_swap(np.zeros((3, N - 1), bool))
  with pytest.raises(ValueError):
    eng.renyi2_swap([[0, N]])
  with pytest.raises(ValueError):
    eng.renyi2_swap([])                                      # no regions
  with pytest.raises(ValueError):
    eng.renyi2_swap(np.zeros((0, N), np.uint8))
  with pytest.raises(ValueError):
    eng.renyi2_swap(REGIONS, which=2)
  with pytest.raises(ValueError):
    eng.renyi2_swap(REGIONS, regions_per_pass=-1)
  # the C entry itself: no regions, a null mask
  dp = eng._lib.vmc_renyi2_swap
  assert dp(eng._ctx, 0, 0, MASKS.astype(np.uint8).ctypes.data_as(dp.argtypes[3]), 0, None, None) == _hip.VMC_ERR_INVALID
  assert dp(eng._ctx, 0, 1, None, 0, None, None) == _hip.VMC_ERR_INVALID
  swap, match = eng.renyi2_swap(REGIONS)                     # ... and the ctx still measures
  assert match[-1] == HALF
  eng.close()
  odd = _engine(b=B + 1)
  odd.set_params(theta); odd.set_configs(_cfg(9, b=B + 1))
  with pytest.raises(ValueError, match='even'):
    odd.renyi2_swap(REGIONS)
  odd.close()
  tanh = VmcEngine(N, B, 2, H, output_activation='tanh', seed=2024)
  tanh.set_params(theta); tanh.set_configs(_cfg(9))
  with pytest.raises(NotImplementedError, match='exp output'):
    tanh.renyi2_swap(REGIONS)
  tanh.close()
  spec = dict(ansatz='fully_connected', num_layers=1, layer_size=H, nonlinearity='relu', output_activation='exp')
  prod = VmcEngine(N, B, 0, 0, ansatz='prod', children=[spec, dict(spec, ansatz='rbm')], seed=2024)
  with pytest.raises(NotImplementedError, match='product ctx'):
    prod.renyi2_swap(REGIONS)
  with pytest.raises(_hip.ComposedFactorError):
    prod.children[0].renyi2_swap(REGIONS)
  prod.close()

"""GPU: dimer-dimer correlations (vmc_dimer_correlations: csrc/vmc_api_measure.hip + dimer.hip; DimerCorrelationEvaluator;
run_dimer_evaluation) against the fp64 oracle tests/dimer_oracle.py.  Families, shapes and per-row bounds are those of
tests/test_gpu_renyi.py: the 4 x 4 torus, N = 16, H = 32, B = 40 chains (no multiple of the 8- or 16-chain tiles).

Bound.  A ratio r = psi(row) / psi(x) is exp of the difference of two fp32 logs ln|psi|, formed in fp64.  With eps_r the
bound the family's own amplitude / logit parity test applies to ln|psi| of row r, the ratio is within
|r| delta, delta = exp(eps_row + eps_x) - 1, of the oracle's.  dd holds r_b (B on x) with weight |s_i s_j / 4| / 2 = 1/8,
r_a (x') with weight |s'_k s'_l / 4| / 2 = 1/8 and r_ab (the double exchange) with weight 1/4; the fp64 fold of B chains
in a fixed order adds B 2^-53 sum |terms|:
  |dd_sum - ref|   <= sum_c (|r_b| delta_b / 8 + |r_a| delta_a / 8 + |r_ab| delta_ab / 4) + B 2^-53 sum_c sum |terms|
  |bond_sum - ref| <= sum_c |r_a| delta_a / 2 + B 2^-53 sum_c sum |terms|
"""
import functools

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from cgs_vmc_amd import lattice
from tests import dimer_oracle as do
from tests import edvec_oracle as eo
from tests import test_gpu_renyi as tr

pytestmark = pytest.mark.gpu
N, H, B = tr.N, tr.H, tr.B
NON_BONDS = [(0, 5), (2, 11)]                              # a diagonal and a pair three steps apart
BONDS34 = [tuple(b) for b in tr.BONDS] + NON_BONDS          # the 32 bonds of the torus and two pairs of sites that are none
assert len(tr.BONDS) == 32 and not set(NON_BONDS) & set(tr.BONDS)


def _pair_list(bonds):
  """For five first bonds a (three bonds of the torus, the two others): a disjoint partner, a partner sharing a site and
  a itself, each as (a, b) and as (b, a)."""
  pairs = []
  for a in (0, 5, 17, 32, 33):
    sa = set(bonds[a])
    disjoint = next(b for b in range(len(bonds)) if not sa & set(bonds[b]))
    sharing = next(b for b in range(len(bonds)) if b != a and len(sa & set(bonds[b])) == 1)
    for b in (disjoint, sharing):
      pairs += [(a, b), (b, a)]
    pairs.append((a, a))
  return pairs


PAIRS = _pair_list(BONDS34)
assert len(PAIRS) == 25 and len(set(PAIRS)) == 25


def _reference(psi, eps, cfg, bonds, pairs):
  """(bond_sum, dd_sum, bond_bound, dd_bound) from the oracle and the bound of this file's docstring."""
  cfg = np.asarray(cfg, np.float32)
  nb = len(cfg)
  own = np.asarray(psi(cfg), np.float64)
  e_x = eps(cfg)
  ulp = nb * 2.0 ** -53

  def delta(rows, r):
    return np.where(r != 0, np.expm1(eps(rows) + e_x), 0.0)
  single = [do.bond_parts(psi, cfg, b, own) for b in bonds]
  d1 = [delta(s['rows'], s['r']) for s in single]
  bond_ref = do.ascending_sums([s['value'] for s in single])
  bond_bound = np.array([(0.5 * np.abs(s['r']) * d).sum() + ulp * ((np.abs(s['zz']) + 0.5 * np.abs(s['r'])) * s['alive']).sum()
                         for s, d in zip(single, d1)])
  values, dd_bound = [], np.zeros(len(pairs))
  for p, (a, b) in enumerate(pairs):
    q = do.dd_parts(psi, cfg, bonds[a], bonds[b], own)
    d2 = delta(q['rows_ab'], q['r_ab'])
    values.append(q['value'])
    dd_bound[p] = (0.125 * np.abs(q['r_b']) * d1[b] + 0.125 * np.abs(q['r_a']) * d1[a] + 0.25 * np.abs(q['r_ab']) * d2).sum() \
        + ulp * np.abs(q['terms']).sum()
  return bond_ref, do.ascending_sums(values), bond_bound, dd_bound


def _check(tag, got, ref, bound):
  err = np.abs(got - ref)
  with np.errstate(divide='ignore', invalid='ignore'):
    rel = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
  k = int(np.argmax(rel))
  print('%s: worst error / bound %.3g (entry %d: error %.3g, bound %.3g, value %.9g)' % (tag, rel[k], k, err[k], bound[k], ref[k]))
  assert np.isfinite(got).all(), tag
  assert (err <= bound).all(), (tag, k, err[k], bound[k])


@pytest.mark.parametrize('ansatz', tr.FAMILIES)
def test_sums_match_the_fp64_oracle(ansatz):
  theta, psi, eps = tr._family(ansatz)
  cfg = tr._cfg(2)
  assert (cfg.sum(1) == 0).all()
  eng = tr._engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg)
  bond_sum, dd_sum = eng.dimer_correlations(BONDS34, PAIRS)
  bond_ref, dd_ref, bond_bound, dd_bound = _reference(psi, eps, cfg, BONDS34, PAIRS)
  _check(ansatz + ' bond_sum', bond_sum, bond_ref, bond_bound)
  _check(ansatz + ' dd_sum', dd_sum, dd_ref, dd_bound)
  # every branch of the estimator is taken by these chains: parallel and antiparallel first bonds, double exchanges
  parts = do.dd_parts(psi, cfg, BONDS34[PAIRS[2][0]], BONDS34[PAIRS[2][1]])
  assert 0 < parts['anti_a'].sum() < B and 0 < parts['anti_b1'].sum() < parts['anti_a'].sum()
  if ansatz == 'ed_vector':
    assert (psi(cfg) == 0).any()                        # chains whose own amplitude vanishes: 0, never NaN
  # the bonds alone; only one of the two outputs
  only, none = eng.dimer_correlations(BONDS34, [])
  np.testing.assert_array_equal(only, bond_sum); assert none.shape == (0,)
  # the supervisor's parameter set measures through the same entry
  eng.set_params(theta, _hip.VMC_OMEGA)
  bond_w, dd_w = eng.dimer_correlations(BONDS34, PAIRS, which=_hip.VMC_OMEGA)
  np.testing.assert_array_equal(bond_w, bond_sum); np.testing.assert_array_equal(dd_w, dd_sum)
  eng.close()


@pytest.mark.parametrize('ansatz', ['fully_connected', 'pbdg', 'ed_vector'])
def test_a_bond_squared_is_three_sixteenths_minus_half_the_bond(ansatz):
  """(S_i . S_j)^2 = 3/16 - (S_i . S_j) / 2: dd_sum(a, a) = 3 B / 16 - bond_sum(a) / 2 for any amplitudes on any chains
  (B counts the chains whose own amplitude does not vanish), within the bounds of the two sums."""
  theta, psi, eps = tr._family(ansatz)
  cfg = tr._cfg(3)
  eng = tr._engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg)
  same = [(a, a) for a in range(len(BONDS34))]
  bond_sum, dd_sum = eng.dimer_correlations(BONDS34, same)
  _, _, bond_bound, dd_bound = _reference(psi, eps, cfg, BONDS34, same)
  alive = float((psi(cfg) != 0).sum())
  assert alive == B or ansatz == 'ed_vector'
  err = np.abs(dd_sum - (3.0 * alive / 16 - 0.5 * bond_sum))
  bound = dd_bound + 0.5 * bond_bound
  print('%s: dd(a, a) vs 3/16 - bond / 2: max error %.3g, worst error / bound %.3g' % (ansatz, err.max(), (err / bound).max()))
  assert (err <= bound).all()
  eng.close()


@functools.lru_cache(maxsize=None)
def _torus_ground_state():
  return eo.vector_from_ed(N, tr.BONDS, 1.0, 1.0)


def test_an_eigenstate_gives_the_energy_and_its_square_on_any_chains():
  """ed_vector loaded with the 4 x 4 ground state (j = 1): H psi = E0 psi on every configuration, so over the 32 bonds
  sum_a bond_sum = B E0 and the sum of dd_sum over all 1,024 ordered pairs = B E0^2 -- no Monte-Carlo error, whatever the
  chains.  Both within the summed bounds."""
  e0, vec, top, bot = _torus_ground_state()
  vec32 = vec.astype(np.float32)
  psi = lambda c: eo.amplitude(vec32.astype(np.float64), c, top, bot)
  eps = tr._edvec_eps(vec32, top, bot)
  bonds = [tuple(b) for b in tr.BONDS]
  pairs = lattice.all_bond_pairs(len(bonds))
  cfg = tr._cfg(4)
  assert (psi(cfg) != 0).all()
  eng = tr._engine('ed_vector')
  eng.set_params(vec32); eng.set_configs(cfg)
  bond_sum, dd_sum = eng.dimer_correlations(bonds)          # pairs = None: all ordered pairs
  assert dd_sum.shape == (1024,)
  bond_ref, dd_ref, bond_bound, dd_bound = _reference(psi, eps, cfg, bonds, pairs.tolist())
  _check('ground state bond_sum', bond_sum, bond_ref, bond_bound)
  _check('ground state dd_sum', dd_sum, dd_ref, dd_bound)
  err_e, err_e2 = abs(bond_sum.sum() - B * e0), abs(dd_sum.sum() - B * e0 * e0)
  print('E0 = %.9f: |sum bond_sum - B E0| = %.3g (bound %.3g), |sum dd_sum - B E0^2| = %.3g (bound %.3g)'
        % (e0, err_e, bond_bound.sum(), err_e2, dd_bound.sum()))
  assert err_e <= bond_bound.sum() and err_e2 <= dd_bound.sum()
  eng.close()


def test_pass_splits_repeats_subsets_and_longer_lists_are_bit_identical_on_70_pairs():
  """70 pairs: more than one 64-thread fold block, no multiple of 64; 64 pairs per pass leaves a pass of 6."""
  rng = np.random.default_rng(6)
  every = lattice.all_bond_pairs(len(BONDS34))
  pairs = every[rng.permutation(len(every))[:70]]
  theta, psi, eps = tr._family('fully_connected')
  cfg = tr._cfg(7)
  eng = tr._engine()
  eng.set_params(theta); eng.set_configs(cfg)
  base = eng.dimer_correlations(BONDS34, pairs)
  bond_ref, dd_ref, bond_bound, dd_bound = _reference(psi, eps, cfg, BONDS34, pairs.tolist())
  _check('70 pairs bond_sum', base[0], bond_ref, bond_bound)
  _check('70 pairs dd_sum', base[1], dd_ref, dd_bound)
  for per in (0, 1, 7, 64):
    for _ in range(2):
      bond_sum, dd_sum = eng.dimer_correlations(BONDS34, pairs, pairs_per_pass=per)
      np.testing.assert_array_equal(bond_sum, base[0], err_msg='pairs_per_pass=%d' % per)
      np.testing.assert_array_equal(dd_sum, base[1], err_msg='pairs_per_pass=%d' % per)
  # a request splits phase 1 too: 34 bonds at 7 per pass are five passes of single exchanges (the last of 6 bonds, written
  # at dimer.bonds + 28, dimer.logit + 28 B) next to the ten passes of 70 pairs -- one `dimer_rows` region per pass
  eng.timing_enable(True); eng.timing_reset()
  bond_sum, dd_sum = eng.dimer_correlations(BONDS34, pairs, pairs_per_pass=7)
  eng.synchronize()
  passes = eng.timing_get('dimer_rows')[1]
  eng.timing_enable(False)
  assert passes - (70 + 6) // 7 == 5, passes
  np.testing.assert_array_equal(bond_sum, base[0]); np.testing.assert_array_equal(dd_sum, base[1])
  # ... nor on which other pairs are in the list, or where
  pick = rng.permutation(70)[:25]
  bond_sum, dd_sum = eng.dimer_correlations(BONDS34, pairs[pick], pairs_per_pass=4)
  np.testing.assert_array_equal(bond_sum, base[0]); np.testing.assert_array_equal(dd_sum, base[1][pick])
  # ... nor on which other bonds are in the list, or where: the same bonds inside a longer list
  longer = [(3, 9), (1, 0), (15, 4)] + list(BONDS34) + [(7, 8)]
  bond_sum, dd_sum = eng.dimer_correlations(longer, pairs + 3, pairs_per_pass=7)
  np.testing.assert_array_equal(bond_sum[3:-1], base[0]); np.testing.assert_array_equal(dd_sum, base[1])
  eng.close()


def _state(eng):
  return (eng.local_energy()[0], eng.get_configs(), eng.step_counter, eng.get_accumulators())


def test_a_measurement_moves_nothing_else():
  theta, _, _ = tr._family('fully_connected')
  eng = tr._engine()
  eng.set_params(theta); eng.set_configs(tr._cfg(6)); eng.set_bonds(tr.BONDS, 1.0, 1.0)
  eng.mc_steps(3 * N)
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  before = _state(eng)
  terms = eng.local_energy_terms()
  eng.dimer_correlations(BONDS34, PAIRS); eng.dimer_correlations(BONDS34, PAIRS, pairs_per_pass=3)
  after = _state(eng)
  for x, y in zip(before, after):
    np.testing.assert_array_equal(x, y)
  for x, y in zip(terms, eng.local_energy_terms()):    # the Hamiltonian's bond set answers as before
    np.testing.assert_array_equal(x, y)
  eng.mc_steps(N)                                      # straight from the sampler's caches into a measurement
  eloc = eng.local_energy()[0]
  eng.mc_steps(N); chains = eng.get_configs()
  eng.close()
  eng = tr._engine()
  eng.set_params(theta); eng.set_configs(tr._cfg(6)); eng.set_bonds(tr.BONDS, 1.0, 1.0)
  eng.mc_steps(3 * N)
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  eng.mc_steps(N)
  eng.dimer_correlations(BONDS34, PAIRS)
  np.testing.assert_array_equal(eng.local_energy()[0], eloc)
  eng.mc_steps(N)                                      # the next sweep's chains, under the pinned seed
  np.testing.assert_array_equal(eng.get_configs(), chains)
  eng.close()
  # two training epochs with and without a measurement between them: the same parameters
  params = []
  for measure in (False, True):
    eng = tr._engine(b=64, seed=77)
    eng.set_params(theta); eng.set_configs(tr._cfg(7, b=64)); eng.set_bonds(tr.BONDS, 1.0, 1.0)
    for epoch in range(2):
      eng.epoch_energy_gradient(2 * N, 3, N, 1e10)
      eng.apply_adam(_hip.VMC_MODE_ENERGY_GRADIENT, 1e-2)
      if measure and epoch == 0:
        eng.dimer_correlations(BONDS34, PAIRS, pairs_per_pass=5)
    params.append((eng.get_params(), eng.get_configs(), eng.step_counter))
    eng.close()
  for x, y in zip(*params):
    np.testing.assert_array_equal(x, y)


@functools.lru_cache(maxsize=None)
def _exact_chain12():
  n = 12
  bonds = lattice.chain_bonds(n)
  e0, vec, top, bot = eo.vector_from_ed(n, bonds, 1.0, 1.0)
  basis = eo.sz0_configurations(n)
  amp = eo.amplitude(vec, basis, top, bot)
  bond = np.array([do.exact_bond(amp, basis, b) for b in bonds])
  dd = np.array([do.exact_dd(amp, basis, bonds[0], b) for b in bonds])
  return e0, bond, dd


def test_evaluator_reproduces_the_exact_values_within_five_sigma(monkeypatch, tmp_path):
  """The 12-site Heisenberg chain's exact ground state (tools/make_ed_vector.py), bond (0, 1) against all 12 bonds.

  Chosen values: batch_size = 1024, num_evaluation_samples = 20, num_monte_carlo_sweeps = 10.  From the oracle on the
  CPU (the full |psi|^2 distribution, checked against 200,000 independent draws): the standard deviation of one chain's
  dd is 0.222 (nearest neighbour) to 0.365 (third neighbour) over the 12 pairs, that of the connected part (dd minus the
  two bond values weighted by the other's mean) 0.183 to 0.243.  20 x 1,024 chains therefore give dd_err of at most about
  0.365 / sqrt(20480) = 0.0026 and connected_err of about 0.243 / sqrt(20480) = 0.0017, with room for the residual
  correlation of consecutive samples (ten sweeps = 120 exchange proposals per chain on 12 sites apart, as in
  tests/test_gpu_corr.py).  The exact connected values are 0.2104 (a == b), -0.1546 (nearest neighbour), 0.0673, -0.0329,
  0.0257, -0.0211, 0.0207 (opposite bond): five sigma = 0.0085 resolves the nearest-neighbour value from zero eighteen
  times over and the smallest one too.  The product of two batch means biases a sample's connected part by
  -cov(bond_a, bond_b) / 1024, below 5e-5: a thirtieth of the error.  Measured on an MI355X with the seeds below: dd_err
  0.0014 to 0.0027, connected_err 0.0011 to 0.0018, the worst of the 24 deviations 1.53 sigma."""
  from cgs_vmc_amd import run_dimer_evaluation as rd, session, wavefunctions
  from tools import make_ed_vector as mk
  n = 12
  e0, bond, dd = _exact_chain12()
  connected = dd - bond[0] * bond
  monkeypatch.setenv('CGS_VMC_SEED', '20241018')
  monkeypatch.setenv('CGS_VMC_CONFIG_SEED', '5')
  d = str(tmp_path / 'ed')
  assert abs(mk.main([d, '--lattice', 'chain', '--size', str(n)]) - e0) < 1e-9
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  result, written = rd.main(['--checkpoint_dir', d, '--hparams',
                             'batch_size=1024,num_evaluation_samples=20,num_monte_carlo_sweeps=10'])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  np.testing.assert_array_equal(result['bonds'], lattice.chain_bonds(n))
  np.testing.assert_array_equal(result['pairs'], [(0, b) for b in range(n)])
  dev_dd = np.abs(result['dd'] - dd) / result['dd_err']
  dev_cn = np.abs(result['connected'] - connected) / result['connected_err']
  dev_b = np.abs(result['bond'] - bond) / result['bond_err']
  for b in range(n):
    print('bond 0 x bond %2d: dd %.5f +/- %.5f (exact %.5f, %.2f sigma), connected %.5f +/- %.5f (exact %.5f, %.2f sigma)'
          % (b, result['dd'][b], result['dd_err'][b], dd[b], dev_dd[b], result['connected'][b], result['connected_err'][b],
             connected[b], dev_cn[b]))
  assert (result['dd_err'] > 0).all() and (result['connected_err'] > 0).all()
  assert (dev_dd <= 5.0).all(), dev_dd
  assert (dev_cn <= 5.0).all(), dev_cn
  assert (dev_b <= 5.0).all(), dev_b
  # resolving power: five sigma separates the nearest-neighbour connected value from zero
  assert 5.0 * result['connected_err'][1] < abs(connected[1]) and 5.0 * result['connected_err'][n - 1] < abs(connected[n - 1])
  assert result['samples'].shape == (20, 2, n) and result['bond_samples'].shape == (20, n)
  # the chain's bonds are known: both files
  assert [p.rsplit('/', 1)[1] for p in written] == ['dimer_correlations.txt', 'dimer_structure_factor.txt']
  rows = np.loadtxt(written[0])
  assert rows.shape == (n, 8) and np.isfinite(rows).all()
  np.testing.assert_allclose(rows[:, 4], result['dd'], rtol=1e-9)
  np.testing.assert_allclose(rows[:, 6], result['connected'], rtol=1e-8, atol=1e-12)
  sq = np.loadtxt(written[1])
  assert sq.shape == (n, 2) and np.isfinite(sq).all()
  # D(q) of one reference bond against all: sum_b cos(q (r_b - r_0)) connected(0, b); staggered correlations peak at q = pi
  q = lattice.chain_momenta(n)[:, 0]                     # (the file's q are rounded to ten digits: the exact ones here)
  np.testing.assert_allclose(sq[:, 0], q, rtol=1e-9)
  np.testing.assert_allclose(sq[:, 1], np.cos(np.outer(q, np.arange(n))) @ result['connected'], rtol=1e-8, atol=1e-12)
  assert np.argmax(sq[:, 1]) == n // 2


def test_cli_on_the_4x4_cluster_writes_both_files(monkeypatch, tmp_path):
  from cgs_vmc_amd import run_dimer_evaluation as rd, session, wavefunctions
  from tools import make_ed_vector as mk
  monkeypatch.setenv('CGS_VMC_SEED', '20241018')
  monkeypatch.setenv('CGS_VMC_CONFIG_SEED', '5')
  d = str(tmp_path / 'ed')
  out = str(tmp_path / 'out')
  mk.main([d, '--lattice', 'square', '--size', '4', '4'])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  result, written = rd.main(['--checkpoint_dir', d, '--output_dir', out, '--reference_bond', '3', '--hparams',
                             'size_x=4,size_y=4,batch_size=256,num_evaluation_samples=6,num_monte_carlo_sweeps=4'])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  assert written == [out + '/dimer_correlations.txt', out + '/dimer_structure_factor.txt']
  bonds = lattice.load_bonds(d, N)
  assert len(bonds) == 32
  rows = np.loadtxt(written[0])
  assert rows.shape == (32, 8) and np.isfinite(rows).all()
  np.testing.assert_array_equal(rows[:, :2], np.repeat([bonds[3]], 32, axis=0))
  np.testing.assert_array_equal(rows[:, 2:4], bonds)
  np.testing.assert_allclose(rows[:, 4], result['dd'], rtol=1e-9)
  np.testing.assert_allclose(rows[:, 5], result['dd_err'], rtol=1e-2)
  np.testing.assert_allclose(rows[:, 6], result['connected'], rtol=1e-8, atol=1e-12)
  np.testing.assert_allclose(rows[:, 7], result['connected_err'], rtol=1e-2)
  assert (rows[:, 5] > 0).all() and (rows[:, 7] > 0).all()
  # the a == a line: dd = 3/16 - bond / 2 within its error; from the line alone, bond^2 = dd - connected with bond < 0
  line = rows[3]
  assert abs(result['dd'][3] - (3.0 / 16 - 0.5 * result['bond'][3])) <= result['dd_err'][3]
  assert line[4] > line[6] and abs(line[4] - (3.0 / 16 + 0.5 * np.sqrt(line[4] - line[6]))) <= line[5]
  sq = np.loadtxt(written[1])
  assert sq.shape == (16, 4) and np.isfinite(sq).all()
  np.testing.assert_allclose(sq[:, :2], lattice.torus_momenta(4, 4), rtol=1e-9)
  qs, dq = lattice.dimer_structure_factor(result['bonds'], result['pairs'], result['connected'], 4, 4)
  np.testing.assert_allclose(sq[:, 2:], dq.T, rtol=1e-8, atol=1e-10)
  axis, _ = lattice.bond_orientations(bonds, 4, 4)
  assert (dq[1 - axis[3]] == 0).all() and (dq[axis[3]] != 0).any()        # the reference bond's orientation alone has pairs


def test_refusals():
  from cgs_vmc_amd.engine import VmcEngine
  theta, psi, eps = tr._family('fully_connected')
  cfg = tr._cfg(9)
  eng = tr._engine()
  eng.set_configs(cfg)
  with pytest.raises(_hip.HipLibraryError, match='parameters not set'):
    eng.dimer_correlations(BONDS34, PAIRS)
  eng.set_params(theta)
  for bad_bonds in ([(0, 1), (3, 3)], [(0, N)], [(-1, 2)], []):      # i == j, a site out of range, no bonds
    with pytest.raises(ValueError):
      eng.dimer_correlations(bad_bonds, [])
  for bad_pairs in ([(0, len(BONDS34))], [(-1, 0)]):                 # a bond index out of range
    with pytest.raises(ValueError):
      eng.dimer_correlations(BONDS34, bad_pairs)
  with pytest.raises(ValueError):
    eng.dimer_correlations(BONDS34, PAIRS, which=2)
  with pytest.raises(ValueError):
    eng.dimer_correlations(BONDS34, PAIRS, which=-1)
  with pytest.raises(ValueError):
    eng.dimer_correlations(BONDS34, PAIRS, pairs_per_pass=-1)
  # the C entry itself: the codes of the table
  fn = eng._lib.vmc_dimer_correlations
  ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(fn.argtypes[3])
  good_b, good_p = np.array(BONDS34, np.int32), np.array(PAIRS, np.int32)
  call = lambda which, nb, b, npairs, p, per: fn(eng._ctx, which, nb, ip(b), npairs, ip(p), per, None, None)
  assert call(0, 2, [(0, 1), (3, 3)], 0, good_p, 0) == _hip.VMC_ERR_INVALID
  assert call(0, 1, [(0, N)], 0, good_p, 0) == _hip.VMC_ERR_INVALID
  assert call(0, 34, good_b, 1, [(0, 34)], 0) == _hip.VMC_ERR_INVALID
  assert call(0, 0, good_b, 0, good_p, 0) == _hip.VMC_ERR_INVALID
  assert call(0, 34, good_b, -1, good_p, 0) == _hip.VMC_ERR_INVALID
  assert call(0, 34, good_b, 25, good_p, -1) == _hip.VMC_ERR_INVALID
  assert call(2, 34, good_b, 25, good_p, 0) == _hip.VMC_ERR_INVALID
  assert fn(eng._ctx, 0, 34, None, 0, None, 0, None, None) == _hip.VMC_ERR_INVALID
  assert fn(eng._ctx, 0, 34, ip(good_b), 25, None, 0, None, None) == _hip.VMC_ERR_INVALID
  assert call(0, 34, good_b, 25, good_p, 0) == _hip.VMC_OK             # both outputs NULL: legal
  # ... and the ctx still measures correctly
  bond_sum, dd_sum = eng.dimer_correlations(BONDS34, PAIRS)
  bond_ref, dd_ref, bond_bound, dd_bound = _reference(psi, eps, cfg, BONDS34, PAIRS)
  _check('after the refusals, bond_sum', bond_sum, bond_ref, bond_bound)
  _check('after the refusals, dd_sum', dd_sum, dd_ref, dd_bound)
  eng.close()
  tanh = VmcEngine(N, B, 2, H, output_activation='tanh', seed=2024)
  tanh.set_params(theta); tanh.set_configs(cfg)
  with pytest.raises(NotImplementedError, match='exp output'):
    tanh.dimer_correlations(BONDS34, PAIRS)
  fn_t = tanh._lib.vmc_dimer_correlations
  assert fn_t(tanh._ctx, 0, 34, ip(good_b), 25, ip(good_p), 0, None, None) == _hip.VMC_ERR_UNSUPPORTED
  tanh.close()
  spec = dict(ansatz='fully_connected', num_layers=1, layer_size=H, nonlinearity='relu', output_activation='exp')
  prod = VmcEngine(N, B, 0, 0, ansatz='prod', children=[spec, dict(spec, ansatz='rbm')], seed=2024)
  with pytest.raises(NotImplementedError, match='product ctx'):
    prod.dimer_correlations(BONDS34, PAIRS)
  assert fn(prod._ctx, 0, 34, ip(good_b), 25, ip(good_p), 0, None, None) == _hip.VMC_ERR_UNSUPPORTED
  with pytest.raises(_hip.ComposedFactorError):
    prod.children[0].dimer_correlations(BONDS34, PAIRS)
  assert fn(prod.children[0]._ctx, 0, 34, ip(good_b), 25, ip(good_p), 0, None, None) == _hip.VMC_ERR_STATE
  prod.close()

"""CPU: the swap-estimator oracle against exact Tr rho_A^2 (singular values) on the 8-site chain's ground state,
lattice.block_regions / read_regions / region_masks, and RenyiEntropyEvaluator's bookkeeping (errors, sharded sums and pair
counts) on an engine double that gets renyi2_swap from the oracle."""
import types

import numpy as np
import pytest

from cgs_vmc_amd import evaluation
from cgs_vmc_amd import lattice
from cgs_vmc_amd import parallel
from cgs_vmc_amd import session as session_lib
from tests import edvec_oracle as eo
from tests import renyi_oracle as ro

N8 = 8
REGIONS8 = lattice.block_regions(N8) + [[1, 4, 6]]           # the blocks l = 1 .. 4 and one scattered region


def _chain_ground_state():
  e0, vec, top, bot = eo.vector_from_ed(N8, lattice.chain_bonds(N8), 1.0, 1.0)
  return (lambda c: eo.amplitude(vec, c, top, bot)), eo.sz0_configurations(N8)


def test_oracle_summed_over_all_pairs_of_basis_states_is_the_exact_purity():
  psi, basis = _chain_ground_state()
  assert len(basis) == 70
  purities = []
  for mask in ro.masks(REGIONS8, N8):
    exact = ro.exact_purity(psi, basis, mask)
    got = ro.exact_swap_expectation(psi, basis, mask)
    print('region %s: swap expectation %.15f, singular values %.15f' % (np.flatnonzero(mask).tolist(), got, exact))
    assert abs(got - exact) <= 1e-12, (mask, got, exact)
    purities.append(exact)
  # a singlet: one site is maximally mixed (Tr rho^2 = 1 / 2)
  assert abs(purities[0] - 0.5) < 1e-12 and all(0.0 < p <= 1.0 for p in purities)
  # the empty and the full region leave a pure state
  for mask in (np.zeros(N8, bool), np.ones(N8, bool)):
    assert abs(ro.exact_purity(psi, basis, mask) - 1.0) < 1e-12
    assert abs(ro.exact_swap_expectation(psi, basis, mask) - 1.0) < 1e-12


def test_oracle_terms_match_rule_zero_amplitudes_and_complement():
  rng = np.random.default_rng(0)
  top, bot, length = eo.lin_tables(N8)
  vec = rng.standard_normal(length)
  vec[rng.integers(0, length, 12)] = 0.0
  psi = lambda c: eo.amplitude(vec, c, top, bot)
  cfg = eo.sz0_configurations(N8)[rng.permutation(70)[:40]]
  masks = ro.masks(REGIONS8 + [[], list(range(N8))], N8)
  terms, match = ro.pair_terms(psi, cfg, masks)
  assert np.isfinite(terms).all() and (terms[~match] == 0).all()
  assert match[-2:].all()                                       # empty and full: every pair matches
  p = psi(cfg)
  full = np.where((p[:20] != 0) & (p[20:] != 0), 1.0, 0.0)      # ... with term 1 (0 where a chain's own amplitude vanishes)
  np.testing.assert_allclose(terms[-1], full, rtol=1e-15)
  np.testing.assert_allclose(terms[-2], full, rtol=1e-15)
  t2, m2 = ro.pair_terms(psi, cfg, ~masks)                      # the complement: the two swapped rows trade places
  np.testing.assert_array_equal(m2, match)
  np.testing.assert_allclose(t2, terms, rtol=1e-14)
  sums, counts = ro.swap_sums(psi, cfg, masks)
  np.testing.assert_allclose(sums, terms.sum(1), rtol=1e-14)
  np.testing.assert_array_equal(counts, match.sum(1))


def test_block_regions_read_regions_and_masks(tmp_path):
  assert lattice.block_regions(8) == [[0], [0, 1], [0, 1, 2], [0, 1, 2, 3]]
  assert lattice.block_regions(7) == [[0], [0, 1], [0, 1, 2]]
  assert lattice.block_regions(6, max_len=5)[-1] == [0, 1, 2, 3, 4] and lattice.block_regions(6, 0) == []
  with pytest.raises(ValueError):
    lattice.block_regions(6, 7)
  f = tmp_path / 'regions.txt'
  f.write_text('# blocks\n0 1\n\n5, 2 3   # scattered\n7\n')
  regions = lattice.read_regions(str(f))
  assert regions == [[0, 1], [5, 2, 3], [7]]
  m = lattice.region_masks(regions, 8)
  assert m.dtype == np.uint8 and m.shape == (3, 8)
  np.testing.assert_array_equal(m, ro.masks(regions, 8))
  np.testing.assert_array_equal(lattice.region_masks(m, 8), m)               # 0/1 arrays pass through
  np.testing.assert_array_equal(lattice.region_masks(m.astype(bool), 8), m)
  np.testing.assert_array_equal(lattice.region_masks([[], range(8)], 8), [[0] * 8, [1] * 8])
  for bad in ([[0, 8]], [[-1]], [[2, 2]], [[0.5]]):
    with pytest.raises(ValueError):
      lattice.region_masks(bad, 8)
  with pytest.raises(ValueError):
    lattice.region_masks(np.zeros((2, 7), np.uint8), 8)                      # a mask of the wrong shape
  with pytest.raises(ValueError):
    lattice.region_masks(np.zeros((2, 7), bool), 8)
  f.write_text('0 1\n2 x\n')
  with pytest.raises(ValueError, match='regions.txt:2'):
    lattice.read_regions(str(f))
  from cgs_vmc_amd import run_entanglement_evaluation as re_
  f.write_text('0 9\n')
  with pytest.raises(ValueError, match='out of range'):
    re_.load_regions(str(f), 8)
  assert re_.load_regions('', 8) == lattice.block_regions(8)


class _OracleEngine:
  """Engine double: a scripted list of chain sets; renyi2_swap is the oracle's on the current set, mc_steps (run_many
  of the sampler op) moves on to the next set after the thermalisation call."""

  def __init__(self, psi, chain_sets):
    self.psi, self.sets, self.at, self.steps, self.calls = psi, list(chain_sets), 0, [], 0
    self.batch_size = len(self.sets[0])

  def renyi2_swap(self, regions, which=0, regions_per_pass=0):
    assert which == 0 and regions_per_pass == 0
    self.calls += 1
    return ro.swap_sums(self.psi, self.sets[self.at], np.asarray(regions, bool))

  def run_many(self, n):
    if self.steps:                                        # (the first call is the thermalisation)
      self.at = min(self.at + 1, len(self.sets) - 1)
    self.steps.append(n)


def _ops(engine, regions):
  mc = session_lib.Op(lambda: None, 'mc_step')
  mc.last_accepted = 3
  mc.run_many = engine.run_many
  value = evaluation.RenyiSwapTensor(engine, regions, 0, N8)
  return evaluation.EvalOps(value=value, mc_step=mc, acceptance_rate=None, placeholder_input=None, wavefunction_value=None)


def _hparams(n_samples, batch):
  return types.SimpleNamespace(num_sites=N8, batch_size=batch, num_equilibration_sweeps=5, num_monte_carlo_sweeps=2,
                               num_evaluation_samples=n_samples)


def _chain_sets(n_sets, batch, seed):
  rng = np.random.default_rng(seed)
  basis = eo.sz0_configurations(N8)
  return [basis[rng.integers(0, len(basis), batch)] for _ in range(n_sets)]


def test_evaluator_dict_and_standard_errors_on_the_oracle_double(monkeypatch):
  psi, _ = _chain_ground_state()
  n_samples, batch = 6, 24
  sets = _chain_sets(n_samples, batch, 1)
  eng = _OracleEngine(psi, sets)
  ev = evaluation.RenyiEntropyEvaluator()
  out = ev.run_evaluation(_ops(eng, REGIONS8), session_lib.Session(), _hparams(n_samples, batch), epoch_num=0)
  assert set(out) == {'regions', 'purity', 'purity_err', 's2', 's2_err', 'match_fraction', 'samples'}
  assert eng.calls == n_samples and eng.steps == [5 * N8] + [2 * N8] * n_samples
  assert ev.acceptance_count == 3 * n_samples
  masks = ro.masks(REGIONS8, N8)
  np.testing.assert_array_equal(out['regions'], masks.astype(np.uint8))
  ref = np.array([ro.swap_sums(psi, s, masks)[0] / (batch // 2) for s in sets])
  frac = np.array([ro.swap_sums(psi, s, masks)[1] / (batch // 2) for s in sets])
  np.testing.assert_allclose(out['samples'], ref, rtol=1e-15)
  np.testing.assert_allclose(out['purity'], ref.mean(0), rtol=1e-14)
  err = np.sqrt(((ref - ref.mean(0)) ** 2).sum(0) / (n_samples - 1) / n_samples)          # per region, by hand
  np.testing.assert_allclose(out['purity_err'], err, rtol=1e-13)
  np.testing.assert_allclose(out['s2'], -np.log(ref.mean(0)), rtol=1e-14)
  np.testing.assert_allclose(out['s2_err'], err / ref.mean(0), rtol=1e-13)
  np.testing.assert_allclose(out['match_fraction'], frac.mean(0), rtol=1e-15)
  assert (out['match_fraction'] > 0).all() and (out['match_fraction'] <= 1).all()
  # a single sample has no spread to report
  one = evaluation.RenyiEntropyEvaluator().run_evaluation(
      _ops(_OracleEngine(psi, sets[:1]), REGIONS8), session_lib.Session(), _hparams(1, batch), epoch_num=0)
  assert (one['purity_err'] == 0).all() and (one['s2_err'] == 0).all()
  np.testing.assert_allclose(one['purity'], ref[0], rtol=1e-15)
  # operator = None means the blocks
  wf = types.SimpleNamespace(_which=0, _bind=lambda configs: eng)
  monkeypatch.setattr(evaluation.graph_builders, 'get_configs', lambda *a, **k: None)
  monkeypatch.setattr(evaluation.graph_builders, 'get_monte_carlo_sampling', lambda *a, **k: (None, None))
  ops = evaluation.RenyiEntropyEvaluator().build_eval_ops(wf, None, _hparams(1, batch), {})
  np.testing.assert_array_equal(ops.value.masks, ro.masks(lattice.block_regions(N8), N8))


def test_evaluator_adds_sharded_sums_and_pair_counts_before_the_division(monkeypatch):
  psi, _ = _chain_ground_state()
  n_samples, local_batch, world = 3, 16, 2
  sets = _chain_sets(n_samples, local_batch, 2)
  masks = ro.masks(REGIONS8, N8)
  # what the second rank adds to every sample: other sums, other match counts, and a DIFFERENT number of pairs
  other = np.stack([np.linspace(1.0, 2.0, len(masks)), np.full(len(masks), 5.0), np.full(len(masks), 12.0)])
  reduced = []

  def fake_allreduce(values, op='sum'):
    values = np.asarray(values, np.float64)
    assert op == 'sum' and values.dtype == np.float64 and values.shape == (3, len(masks))
    reduced.append(values.copy())
    return values + other
  monkeypatch.setattr(parallel, 'world_size', lambda: world)
  monkeypatch.setattr(parallel, 'allreduce_array', fake_allreduce)
  out = evaluation.RenyiEntropyEvaluator().run_evaluation(
      _ops(_OracleEngine(psi, sets), REGIONS8), session_lib.Session(), _hparams(n_samples, world * local_batch), epoch_num=0)
  assert len(reduced) == n_samples                      # one collective per sample, on the fp64 sums and counts
  fracs = []
  for s in range(n_samples):
    swap, match = ro.swap_sums(psi, sets[s], masks)
    np.testing.assert_array_equal(reduced[s], np.stack([swap, match, np.full(len(masks), local_batch // 2)]))
    pairs = local_batch // 2 + other[2]
    np.testing.assert_allclose(out['samples'][s], (swap + other[0]) / pairs, rtol=1e-15)
    fracs.append((match + other[1]) / pairs)
  np.testing.assert_allclose(out['match_fraction'], np.mean(fracs, 0), rtol=1e-15)
  # single rank: no collective at all
  reduced.clear()
  monkeypatch.setattr(parallel, 'world_size', lambda: 1)
  evaluation.RenyiEntropyEvaluator().run_evaluation(
      _ops(_OracleEngine(psi, sets), REGIONS8), session_lib.Session(), _hparams(n_samples, local_batch), epoch_num=0)
  assert reduced == []


def test_entanglement_file_has_one_line_per_region(tmp_path):
  from cgs_vmc_amd import run_entanglement_evaluation as re_
  masks = ro.masks(REGIONS8, N8).astype(np.uint8)
  k = len(masks)
  purity = np.linspace(0.5, 0.3, k)
  result = {'regions': masks, 'purity': purity, 'purity_err': np.full(k, 1e-3), 's2': -np.log(purity),
            's2_err': 1e-3 / purity, 'match_fraction': np.linspace(0.5, 0.25, k)}
  rows = np.loadtxt(re_.write_entanglement(str(tmp_path), result))
  assert rows.shape == (k, 6)
  np.testing.assert_array_equal(rows[:, 0], masks.sum(1))
  np.testing.assert_allclose(rows[:, 1], purity, rtol=1e-9)
  np.testing.assert_allclose(rows[:, 3], -np.log(purity), rtol=1e-9)
  np.testing.assert_allclose(rows[:, 4], 1e-3 / purity, rtol=1e-2)

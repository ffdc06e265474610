"""CPU: the spin-correlation oracle against brute force, lattice.structure_factor on two exact cases, and
SpinCorrelationEvaluator's bookkeeping (errors, sharded sums, the global batch) on an engine stub."""
import itertools
import types

import numpy as np
import pytest

from cgs_vmc_amd import evaluation
from cgs_vmc_amd import lattice
from cgs_vmc_amd import parallel
from cgs_vmc_amd import session as session_lib
from tests import corr_oracle as co
from tests import exact_states


def test_oracle_matches_dense_spin_matrices_on_an_explicit_8_site_vector():
  n = 8
  rng = np.random.default_rng(0)
  vec = rng.standard_normal(1 << n)                    # every Sz sector, both signs
  vec[rng.integers(0, 1 << n, 9)] = 0.0                # and zeros (neighbours of zeros still count)
  pairs = lattice.all_pairs(n)
  got = co.expectation(co.vector_psi(vec), co.all_configurations(n), pairs)
  for k, (i, j) in enumerate(pairs):
    ref = vec @ co.dense_ss_matrix(n, i, j) @ vec / (vec @ vec)
    assert abs(got[k] - ref) < 1e-13, (i, j, got[k], ref)


def test_pair_sums_are_the_sums_of_pair_terms():
  n = 6
  vec = np.random.default_rng(1).uniform(0.5, 1.5, 1 << n)
  cfg = co.all_configurations(n)[[5, 9, 9, 33, 62]]
  pairs = [(0, 1), (4, 2), (5, 0)]
  sz, ratio = co.pair_terms(co.vector_psi(vec), cfg, pairs)
  assert set(np.unique(sz)) <= {-1.0, 1.0} and (ratio[sz > 0] == 0).all() and (ratio[sz < 0] > 0).all()
  zz, ex = co.pair_sums(co.vector_psi(vec), cfg, pairs)
  np.testing.assert_array_equal(zz, sz.sum(0))
  szsz, exch, ss = co.pair_means(co.vector_psi(vec), cfg, pairs)
  np.testing.assert_allclose(ss, (0.25 * sz + 0.5 * ratio).mean(0), rtol=1e-15)
  np.testing.assert_allclose(szsz + exch, ss, rtol=1e-15)


def test_all_pairs_and_coordinates():
  p = lattice.all_pairs(5)
  assert p.dtype == np.int32 and p.shape == (10, 2)
  assert [tuple(x) for x in p] == list(itertools.combinations(range(5), 2))
  xy = lattice.torus_coords(4, 3)
  for i, j in lattice.torus_bonds(4, 3):                # neighbours of torus_bonds are one step apart on the torus
    d = np.abs(xy[i] - xy[j])
    d = np.minimum(d, np.array([4, 3]) - d)
    assert d.sum() == 1
  assert lattice.chain_coords(6).shape == (6, 1) and lattice.chain_momenta(6).shape == (6, 1)
  q = lattice.torus_momenta(4, 2)
  assert q.shape == (8, 2) and np.allclose(q[5], [2 * np.pi / 4, np.pi])


@pytest.mark.parametrize('shape', [(8,), (4, 4), (4, 2)])
def test_structure_factor_of_the_neel_product_state(shape):
  """<S_i . S_j> = s_i s_j / 4 on a product state: S(Q) = (N + 2) / 4 at the ordering vector, 1 / 2 at every other allowed q."""
  if len(shape) == 1:
    coords, qs = lattice.chain_coords(shape[0]), lattice.chain_momenta(shape[0])
  else:
    coords, qs = lattice.torus_coords(*shape), lattice.torus_momenta(*shape)
  n = len(coords)
  neel = co.neel_configuration(coords)
  pairs = lattice.all_pairs(n)
  ss = 0.25 * neel[pairs[:, 0]] * neel[pairs[:, 1]]
  # the same from the oracle: a vector with one nonzero entry
  vec = np.zeros(1 << n); vec[int((neel > 0) @ (1 << np.arange(n)))] = 1.0
  np.testing.assert_allclose(co.expectation(co.vector_psi(vec), neel[None], pairs), ss, atol=0)
  s_q = lattice.structure_factor(ss, pairs, coords, qs)
  at_q = np.all(np.isclose(qs, np.pi), axis=1)
  assert at_q.sum() == 1
  np.testing.assert_allclose(s_q[at_q], (n + 2) / 4.0, rtol=1e-13)
  np.testing.assert_allclose(s_q[~at_q], 0.5, rtol=1e-12)
  # pair order and orientation do not matter
  perm = np.random.default_rng(2).permutation(len(pairs))
  np.testing.assert_allclose(lattice.structure_factor(ss[perm], pairs[perm][:, ::-1], coords, qs), s_q, rtol=1e-12)


def test_structure_factor_of_an_exact_singlet_vanishes_at_q_0():
  """The 8-site Heisenberg chain's ground state has S_tot = 0: S(q = 0) = <S_tot^2> / N = 0, and sum_{i<j} <S_i . S_j> = -3 N / 8."""
  n = 8
  bonds = lattice.chain_bonds(n)
  e0, vec, cfgs, index = exact_states.ed_ground_state(n, bonds, 1.0, 1.0)
  lookup = {tuple(np.flatnonzero(c < 0)): k for k, c in enumerate(cfgs)}
  psi = lambda c: np.array([vec[lookup[tuple(np.flatnonzero(r < 0))]] for r in np.asarray(c)])
  pairs = lattice.all_pairs(n)
  ss = co.expectation(psi, cfgs, pairs)
  assert abs(ss.sum() + 3 * n / 8.0) < 1e-12
  s_q = lattice.structure_factor(ss, pairs, lattice.chain_coords(n), lattice.chain_momenta(n))
  assert abs(s_q[0]) < 1e-12 and (s_q[1:] > 0).all()
  nn = np.array([ss[[k for k, p in enumerate(pairs) if set(p) == {i, j}][0]] for i, j in bonds])
  assert abs(nn.sum() - e0) < 1e-10                     # the nearest-neighbour sum is the energy (J = 1)
  with pytest.raises(ValueError):
    lattice.structure_factor(ss[:-1], pairs, lattice.chain_coords(n), lattice.chain_momenta(n))


class _StubEngine:
  """pair_correlations returns scripted (zz_sum, ex_sum); mc_steps only counts."""

  def __init__(self, script):
    self.script, self.calls, self.steps = list(script), 0, []

  def pair_correlations(self, pairs, which=0, pairs_per_pass=0):
    assert which == 0 and pairs_per_pass == 0
    out = self.script[self.calls]
    self.calls += 1
    return out


def _stub_ops(engine, pairs, global_batch):
  mc = session_lib.Op(lambda: None, 'mc_step')
  mc.last_accepted = 3
  mc.run_many = engine.steps.append
  value = evaluation.PairCorrelationTensor(engine, pairs, 0, global_batch)
  return evaluation.EvalOps(value=value, mc_step=mc, acceptance_rate=None, placeholder_input=None, wavefunction_value=None)


def _hparams(n_samples):
  return types.SimpleNamespace(num_sites=6, batch_size=8, num_equilibration_sweeps=5, num_monte_carlo_sweeps=2,
                               num_evaluation_samples=n_samples)


def test_evaluator_means_and_standard_errors_on_a_stub():
  rng = np.random.default_rng(3)
  pairs = [(0, 1), (2, 5), (4, 3)]
  n_samples, batch = 7, 8
  script = [(rng.integers(-batch, batch + 1, 3).astype(np.float64), rng.standard_normal(3)) for _ in range(n_samples)]
  eng = _StubEngine(script)
  ev = evaluation.SpinCorrelationEvaluator()
  out = ev.run_evaluation(_stub_ops(eng, pairs, batch), session_lib.Session(), _hparams(n_samples), epoch_num=0)
  assert eng.calls == n_samples
  assert eng.steps == [5 * 6] + [2 * 6] * n_samples       # equilibration, then one decorrelation block per sample
  assert ev.acceptance_count == 3 * n_samples
  zz = np.array([s[0] for s in script]); ex = np.array([s[1] for s in script])
  ref = {'szsz': 0.25 * zz / batch, 'exchange': 0.5 * ex / batch, 'ss': (0.25 * zz + 0.5 * ex) / batch}
  np.testing.assert_array_equal(out['pairs'], np.asarray(pairs, np.int32))
  for name, samples in ref.items():
    np.testing.assert_allclose(out[name], samples.mean(0), rtol=1e-14, atol=1e-16)
    err = np.sqrt(((samples - samples.mean(0)) ** 2).sum(0) / (n_samples - 1) / n_samples)      # per pair, by hand
    np.testing.assert_allclose(out[name + '_err'], err, rtol=1e-13, atol=1e-16)
  assert out['samples'].shape == (n_samples, 3, 3)
  one = evaluation.SpinCorrelationEvaluator().run_evaluation(
      _stub_ops(_StubEngine(script[:1]), pairs, batch), session_lib.Session(), _hparams(1), epoch_num=0)
  assert (one['ss_err'] == 0).all()


def test_evaluator_reduces_sharded_sums_once_per_sample_and_divides_by_the_global_batch(monkeypatch):
  pairs = [(0, 1), (1, 2)]
  n_samples, local_batch, world = 4, 8, 2
  script = [(np.array([2.0 * s, -4.0]), np.array([1.0, 0.5 * s])) for s in range(n_samples)]
  other = (np.array([6.0, 2.0]), np.array([-1.0, 3.0]))        # what the second rank adds to every sample
  reduced = []

  def fake_allreduce(values, op='sum'):
    values = np.asarray(values, np.float64)
    assert op == 'sum' and values.dtype == np.float64 and values.shape == (2, 2)
    reduced.append(values.copy())
    return values + np.stack(other)
  monkeypatch.setattr(parallel, 'world_size', lambda: world)
  monkeypatch.setattr(parallel, 'allreduce_array', fake_allreduce)
  eng = _StubEngine(script)
  out = evaluation.SpinCorrelationEvaluator().run_evaluation(
      _stub_ops(eng, pairs, world * local_batch), session_lib.Session(), _hparams(n_samples), epoch_num=0)
  assert len(reduced) == n_samples                      # one collective per sample, on the fp64 sums
  for s in range(n_samples):
    np.testing.assert_array_equal(reduced[s], np.stack(script[s]))
    zz, ex = script[s][0] + other[0], script[s][1] + other[1]
    np.testing.assert_allclose(out['samples'][s, 2], (0.25 * zz + 0.5 * ex) / (world * local_batch), rtol=1e-15)
  # single rank: no collective at all
  reduced.clear()
  monkeypatch.setattr(parallel, 'world_size', lambda: 1)
  evaluation.SpinCorrelationEvaluator().run_evaluation(
      _stub_ops(_StubEngine(script), pairs, local_batch), session_lib.Session(), _hparams(n_samples), epoch_num=0)
  assert reduced == []


def test_correlation_cli_helpers_write_and_read_back(tmp_path):
  from cgs_vmc_amd import run_correlation_evaluation as rc
  pairs = lattice.all_pairs(4)
  result = {'pairs': pairs, 'szsz': np.arange(6) * 0.01, 'exchange': -np.arange(6) * 0.02, 'ss': -np.arange(6) * 0.01,
            'ss_err': np.full(6, 1e-3)}
  path = rc.write_correlations(str(tmp_path), result)
  rows = np.loadtxt(path)
  assert rows.shape == (6, 6)
  np.testing.assert_array_equal(rows[:, :2], pairs)
  np.testing.assert_allclose(rows[:, 2:], np.stack([result['szsz'], result['exchange'], result['ss'], result['ss_err']], 1))
  pf = tmp_path / 'pairs.txt'
  pf.write_text('0 3\n2 1 9.5\n')
  np.testing.assert_array_equal(rc.load_pairs(str(pf), 4), [[0, 3], [2, 1]])
  np.testing.assert_array_equal(rc.load_pairs('', 4), pairs)
  # which lattice the momenta belong to
  hp = types.SimpleNamespace(num_sites=16, size_x=4, size_y=4)
  coords, qs = rc.lattice_geometry(hp, lattice.torus_bonds(4, 4))
  assert coords.shape == (16, 2) and qs.shape == (16, 2)
  hp = types.SimpleNamespace(num_sites=6, size_x=1, size_y=1)
  coords, qs = rc.lattice_geometry(hp, lattice.chain_bonds(6))
  assert coords.shape == (6, 1) and qs.shape == (6, 1)
  assert rc.lattice_geometry(hp, [(0, 2), (1, 3)]) is None

"""CPU: the dimer-dimer oracle against exact <A B> and two operator identities on the 8-site chain's ground state,
DimerCorrelationEvaluator's bookkeeping (connected part per sample, errors, sharded sums) on the oracle-backed engine
double, lattice.dimer_structure_factor on a hand-built columnar pattern, and the file readers."""
import types

import numpy as np
import pytest

from cgs_vmc_amd import evaluation
from cgs_vmc_amd import lattice
from cgs_vmc_amd import parallel
from cgs_vmc_amd import session as session_lib
from oracle import vmc_oracle as vo
from tests import dimer_oracle as do
from tests import edvec_oracle as eo
from tests.oracle_engine import OracleEngine

N8 = 8
BONDS8 = lattice.chain_bonds(N8)
EXTRA8 = [(0, 2), (1, 6)]                                  # two pairs of sites that are no bonds of the chain


def _chain_ground_state():
  e0, vec, top, bot = eo.vector_from_ed(N8, BONDS8, 1.0, 1.0)
  basis = eo.sz0_configurations(N8)
  return e0, (lambda c: eo.amplitude(vec, c, top, bot)), basis, eo.amplitude(vec, basis, top, bot)


def test_estimator_over_the_full_distribution_is_the_exact_expectation():
  e0, psi, basis, amp = _chain_ground_state()
  assert len(basis) == 70 and (amp != 0).all()
  bonds = BONDS8 + EXTRA8
  pairs = lattice.all_bond_pairs(len(bonds))              # disjoint, sharing a site, a == b, (a, b) and (b, a)
  w = amp ** 2 / (amp ** 2).sum()
  dd = do.dd_values(psi, basis, bonds, pairs) @ w
  bond = do.bond_values(psi, basis, bonds) @ w
  worst = 0.0
  for p, (a, b) in enumerate(pairs):
    ref = do.exact_dd(amp, basis, bonds[a], bonds[b])
    worst = max(worst, abs(dd[p] - ref))
    assert abs(dd[p] - ref) < 1e-13, (a, b, dd[p], ref)
  for a, b in enumerate(bonds):
    assert abs(bond[a] - do.exact_bond(amp, basis, b)) < 1e-13
  print('worst |estimator - exact <A B>| over %d pairs: %.3g' % (len(pairs), worst))
  assert abs(bond[:N8].sum() - e0) < 1e-12                # the bonds of the chain add up to the energy (J = 1)
  # A B and B A have the same expectation in a real state although their local values differ
  dd2 = dd.reshape(len(bonds), len(bonds))
  np.testing.assert_allclose(dd2, dd2.T, atol=1e-13)
  vals = do.dd_values(psi, basis, bonds, [(0, 1), (1, 0)])
  assert np.abs(vals[0] - vals[1]).max() > 1e-3


def test_identities_on_every_configuration():
  e0, psi, basis, amp = _chain_ground_state()
  # an eigenstate: <x| H H |psi> / psi(x) = E0^2 on EVERY configuration, H the sum of the chain's bonds
  total = do.dd_values(psi, basis, BONDS8, lattice.all_bond_pairs(N8)).sum(0)
  np.testing.assert_allclose(total, e0 ** 2, rtol=0, atol=1e-11)
  np.testing.assert_allclose(do.bond_values(psi, basis, BONDS8).sum(0), e0, rtol=0, atol=1e-12)
  # (S_i . S_j)^2 = 3/16 - (S_i . S_j) / 2 for two spins 1/2: for ANY amplitudes, on every configuration
  rng = np.random.default_rng(3)
  top, bot, length = eo.lin_tables(N8)
  vec = rng.standard_normal(length)
  rnd = lambda c: eo.amplitude(vec, c, top, bot)
  bonds = BONDS8 + EXTRA8
  same = [(a, a) for a in range(len(bonds))]
  for f in (psi, rnd):
    np.testing.assert_allclose(do.dd_values(f, basis, bonds, same), 3.0 / 16 - 0.5 * do.bond_values(f, basis, bonds),
                               rtol=0, atol=1e-12)
  # a bond written the other way round is the same operator
  np.testing.assert_allclose(do.dd_values(rnd, basis, [(0, 1), (1, 0), (1, 2), (2, 1)], [(0, 2), (1, 3), (0, 3)]),
                             np.repeat(do.dd_values(rnd, basis, [(0, 1), (1, 2)], [(0, 1)]), 3, axis=0), rtol=0, atol=1e-13)


def test_zero_amplitudes_give_zero_terms_never_nan():
  rng = np.random.default_rng(4)
  top, bot, length = eo.lin_tables(N8)
  vec = rng.standard_normal(length)
  vec[::3] = 0.0
  psi = lambda c: eo.amplitude(vec, c, top, bot)
  basis = eo.sz0_configurations(N8)
  bonds = BONDS8 + EXTRA8
  pairs = lattice.all_bond_pairs(len(bonds))
  dd = do.dd_values(psi, basis, bonds, pairs)
  bond = do.bond_values(psi, basis, bonds)
  dead = psi(basis) == 0
  assert dead.any() and np.isfinite(dd).all() and np.isfinite(bond).all()
  assert (dd[:, dead] == 0).all() and (bond[:, dead] == 0).all()
  # summed against |psi|^2 the zeros cost nothing: still the exact expectation
  amp = psi(basis)
  w = amp ** 2 / (amp ** 2).sum()
  for p in (1, 13, 37, 99):
    a, b = pairs[p]
    assert abs(dd[p] @ w - do.exact_dd(amp, basis, bonds[a], bonds[b])) < 1e-13
  bs, ds = do.dimer_sums(psi, basis[:20], bonds, pairs[:7])
  np.testing.assert_allclose(bs, bond[:, :20].sum(1), rtol=1e-14, atol=1e-15)
  np.testing.assert_allclose(ds, dd[:7, :20].sum(1), rtol=1e-14, atol=1e-15)


class _DimerOracleEngine(OracleEngine):
  """tests/oracle_engine.py with the measurement this file is about: dimer_correlations from the fp64 oracle on the
  double's current chains; run_many is its sampler."""

  def __init__(self, *a, **k):
    super(_DimerOracleEngine, self).__init__(*a, **k)
    self.calls, self.steps, self.seen = 0, [], []

  def _psi(self, which=0):
    return lambda c: vo.fc_psi(self.theta[which], c, self.layer_size, self.num_layers, dtype=np.float64)

  def dimer_correlations(self, bonds, pairs=None, which=0, pairs_per_pass=0):
    assert pairs_per_pass == 0
    self.calls += 1
    self.seen.append(self.configs.copy())
    bonds = np.asarray(bonds).reshape(-1, 2)
    pairs = lattice.all_bond_pairs(len(bonds)) if pairs is None else np.asarray(pairs).reshape(-1, 2)
    return do.dimer_sums(self._psi(which), self.configs, bonds.tolist(), pairs.tolist())

  def run_many(self, n):
    self.steps.append(n)
    self.mc_steps(n)


def _double(batch, seed=0):
  h = 8
  eng = _DimerOracleEngine(N8, batch, 1, h)
  eng.set_params(vo.init_params(N8, h, 1, np.random.default_rng(seed)))
  eng.set_configs(vo.random_configurations(N8, batch, np.random.RandomState(seed + 1)))
  return eng


def _ops(engine, bonds, pairs, global_batch):
  mc = session_lib.Op(lambda: None, 'mc_step')
  mc.last_accepted = 3
  mc.run_many = engine.run_many
  value = evaluation.DimerCorrelationTensor(engine, bonds, pairs, 0, global_batch)
  return evaluation.EvalOps(value=value, mc_step=mc, acceptance_rate=None, placeholder_input=None, wavefunction_value=None)


def _hparams(n_samples, batch, **kw):
  return types.SimpleNamespace(num_sites=N8, batch_size=batch, num_equilibration_sweeps=2, num_monte_carlo_sweeps=1,
                               num_evaluation_samples=n_samples, **kw)


PAIRS8 = [(0, 0), (0, 1), (1, 0), (0, 4), (2, 9), (8, 8)]


def test_evaluator_dict_and_standard_errors_on_the_oracle_double(monkeypatch, tmp_path):
  n_samples, batch = 4, 12
  bonds = BONDS8 + EXTRA8
  eng = _double(batch)
  ev = evaluation.DimerCorrelationEvaluator()
  out = ev.run_evaluation(_ops(eng, bonds, PAIRS8, batch), session_lib.Session(), _hparams(n_samples, batch), epoch_num=0)
  assert set(out) == {'bonds', 'pairs', 'bond', 'bond_err', 'dd', 'dd_err', 'connected', 'connected_err', 'samples',
                      'bond_samples'}
  assert eng.calls == n_samples and eng.steps == [2 * N8] + [N8] * n_samples
  assert ev.acceptance_count == 3 * n_samples
  np.testing.assert_array_equal(out['bonds'], bonds); np.testing.assert_array_equal(out['pairs'], PAIRS8)
  assert any((eng.seen[0] != eng.seen[1]).ravel())         # the double's sampler moved the chains between samples
  psi = eng._psi()
  bond = np.array([do.bond_values(psi, s, bonds).mean(1) for s in eng.seen])
  dd = np.array([do.dd_values(psi, s, bonds, PAIRS8).mean(1) for s in eng.seen])
  pa, pb = np.array(PAIRS8).T
  conn = dd - bond[:, pa] * bond[:, pb]                    # per sample, from that sample's batch means
  np.testing.assert_allclose(out['bond_samples'], bond, rtol=1e-13)
  np.testing.assert_allclose(out['samples'][:, 0], dd, rtol=1e-13, atol=1e-15)
  np.testing.assert_allclose(out['samples'][:, 1], conn, rtol=1e-12, atol=1e-15)
  for name, ref in (('bond', bond), ('dd', dd), ('connected', conn)):
    np.testing.assert_allclose(out[name], ref.mean(0), rtol=1e-12, atol=1e-15)
    err = np.sqrt(((ref - ref.mean(0)) ** 2).sum(0) / (n_samples - 1) / n_samples)       # by hand
    np.testing.assert_allclose(out[name + '_err'], err, rtol=1e-10, atol=1e-15)
  # a == a obeys 3/16 - bond / 2 sample by sample
  np.testing.assert_allclose(out['samples'][:, 0, 0], 3.0 / 16 - 0.5 * out['bond_samples'][:, 0], rtol=0, atol=1e-13)
  # a single sample has no spread to report
  one = evaluation.DimerCorrelationEvaluator().run_evaluation(
      _ops(_double(batch), bonds, PAIRS8, batch), session_lib.Session(), _hparams(1, batch), epoch_num=0)
  assert (one['dd_err'] == 0).all() and (one['connected_err'] == 0).all() and (one['bond_err'] == 0).all()
  np.testing.assert_allclose(one['dd'], dd[0], rtol=1e-13, atol=1e-15)
  # pairs = None: all ordered pairs; operator = None: the bonds of J.txt (else the chain), each paired with bond 0
  t = evaluation.DimerCorrelationTensor(eng, bonds, None, 0, batch)
  np.testing.assert_array_equal(t.pairs, lattice.all_bond_pairs(len(bonds)))
  wf = types.SimpleNamespace(_which=0, _bind=lambda configs: eng)
  monkeypatch.setattr(evaluation.graph_builders, 'get_configs', lambda *a, **k: None)
  monkeypatch.setattr(evaluation.graph_builders, 'get_monte_carlo_sampling', lambda *a, **k: (None, None))
  ops = evaluation.DimerCorrelationEvaluator().build_eval_ops(wf, None, _hparams(1, batch, checkpoint_dir=str(tmp_path)), {})
  np.testing.assert_array_equal(ops.value.bonds, BONDS8)
  np.testing.assert_array_equal(ops.value.pairs, [(0, b) for b in range(N8)])
  lattice.write_bonds(str(tmp_path), [(0, 1), (2, 5), (3, 4)])
  ops = evaluation.DimerCorrelationEvaluator().build_eval_ops(wf, None, _hparams(1, batch, checkpoint_dir=str(tmp_path)), {})
  np.testing.assert_array_equal(ops.value.bonds, [(0, 1), (2, 5), (3, 4)])
  np.testing.assert_array_equal(ops.value.pairs, [(0, 0), (0, 1), (0, 2)])
  with pytest.raises(ValueError):
    evaluation.DimerCorrelationTensor(eng, bonds, [(0, len(bonds))], 0, batch)
  with pytest.raises(ValueError):
    evaluation.DimerCorrelationTensor(eng, [], [], 0, batch)


def test_evaluator_adds_sharded_sums_before_the_division(monkeypatch):
  n_samples, local_batch, world = 2, 6, 2
  bonds = BONDS8 + EXTRA8
  other = np.linspace(-1.0, 2.0, len(bonds) + len(PAIRS8))     # what the second rank adds to every sample
  reduced = []

  def fake_allreduce(values, op='sum'):
    values = np.asarray(values, np.float64)
    assert op == 'sum' and values.dtype == np.float64 and values.shape == other.shape
    reduced.append(values.copy())
    return values + other
  monkeypatch.setattr(parallel, 'world_size', lambda: world)
  monkeypatch.setattr(parallel, 'allreduce_array', fake_allreduce)
  eng = _double(local_batch, seed=5)
  out = evaluation.DimerCorrelationEvaluator().run_evaluation(
      _ops(eng, bonds, PAIRS8, world * local_batch), session_lib.Session(), _hparams(n_samples, world * local_batch), epoch_num=0)
  assert len(reduced) == n_samples                       # one collective per sample, on the fp64 sums
  pa, pb = np.array(PAIRS8).T
  for s in range(n_samples):
    bs, ds = do.dimer_sums(eng._psi(), eng.seen[s], bonds, PAIRS8)
    np.testing.assert_array_equal(reduced[s], np.concatenate([bs, ds]))
    bond = (bs + other[:len(bonds)]) / (world * local_batch)
    dd = (ds + other[len(bonds):]) / (world * local_batch)
    np.testing.assert_allclose(out['bond_samples'][s], bond, rtol=1e-15)
    np.testing.assert_allclose(out['samples'][s, 0], dd, rtol=1e-15)
    np.testing.assert_allclose(out['samples'][s, 1], dd - bond[pa] * bond[pb], rtol=1e-13, atol=1e-16)
  # single rank: no collective at all
  reduced.clear()
  monkeypatch.setattr(parallel, 'world_size', lambda: 1)
  evaluation.DimerCorrelationEvaluator().run_evaluation(
      _ops(_double(local_batch), bonds, PAIRS8, local_batch), session_lib.Session(), _hparams(n_samples, local_batch), epoch_num=0)
  assert reduced == []


def test_bond_orientations_on_torus_and_chain():
  bonds = lattice.torus_bonds(4, 3)
  axis, origin = lattice.bond_orientations(bonds, 4, 3)
  np.testing.assert_array_equal(axis, [0, 1] * 12)        # torus_bonds lists (x bond, y bond) per site
  np.testing.assert_array_equal(origin, np.repeat(np.arange(12), 2))
  flipped = [(j, i) for i, j in bonds]                    # the orientation of the pair does not matter
  np.testing.assert_array_equal(lattice.bond_orientations(flipped, 4, 3)[1], origin)
  axis, origin = lattice.bond_orientations([(0, 5), (0, 2), (3, 0), (0, 8)], 4, 3)
  np.testing.assert_array_equal(axis, [-1, -1, 0, 1]); np.testing.assert_array_equal(origin, [-1, -1, 3, 8])
  axis, origin = lattice.bond_orientations(lattice.chain_bonds(6) + [(0, 3)], 6)
  np.testing.assert_array_equal(axis, [0] * 6 + [-1]); np.testing.assert_array_equal(origin, list(range(6)) + [-1])


@pytest.mark.parametrize('reference_only', [False, True])
def test_dimer_structure_factor_of_a_columnar_pattern(reference_only):
  """Columnar order of x dimers on the 4 x 4 torus: <B_x(r)> = c + d (-1)^x, so the connected part of two x bonds is
  d^2 (-1)^(x_a - x_b) and nothing else correlates: D_x(q) = N d^2 at q = (pi, 0) and 0 at the 15 other momenta, D_y = 0."""
  lx = ly = 4
  d = 0.125
  bonds = lattice.torus_bonds(lx, ly) + [(0, 5), (2, 8)]               # the 32 bonds and two pairs that are none
  axis, origin = lattice.bond_orientations(bonds, lx, ly)
  pairs = lattice.all_bond_pairs(len(bonds))
  if reference_only:
    pairs = pairs[pairs[:, 0] == 2]                                    # bond 2 = the x bond leaving site 1
  a, b = pairs[:, 0], pairs[:, 1]
  both_x = (axis[a] == 0) & (axis[b] == 0)
  connected = np.where(both_x, d * d * (-1.0) ** ((origin[a] % lx) - (origin[b] % lx)), 0.0)
  rng = np.random.default_rng(8)
  mixed = (axis[a] != axis[b]) | (axis[a] < 0)
  connected[mixed] = rng.standard_normal(int(mixed.sum()))             # what must not enter: x-y pairs and non-bonds
  qs, dq = lattice.dimer_structure_factor(bonds, pairs, connected, lx, ly)
  assert qs.shape == (16, 2) and dq.shape == (2, 16)
  np.testing.assert_array_equal(qs, lattice.torus_momenta(lx, ly))
  at = np.isclose(qs[:, 0], np.pi) & np.isclose(qs[:, 1], 0.0)
  assert at.sum() == 1
  np.testing.assert_allclose(dq[0, at], lx * ly * d * d, rtol=1e-13)
  np.testing.assert_allclose(dq[0, ~at], 0.0, atol=1e-14)
  np.testing.assert_allclose(dq[1], 0.0, atol=0)
  # the order of the pairs does not matter
  perm = rng.permutation(len(pairs))
  np.testing.assert_allclose(lattice.dimer_structure_factor(bonds, pairs[perm], connected[perm], lx, ly)[1], dq, atol=1e-14)


def test_dimer_structure_factor_of_a_dimerised_chain_and_its_refusals():
  n, d = 8, 0.25
  bonds = lattice.chain_bonds(n)
  pairs = lattice.all_bond_pairs(n)
  connected = d * d * (-1.0) ** (pairs[:, 0] - pairs[:, 1])
  qs, dq = lattice.dimer_structure_factor(bonds, pairs, connected, n)
  assert qs.shape == (n, 1) and dq.shape == (1, n)
  np.testing.assert_allclose(dq[0, n // 2], n * d * d, rtol=1e-13)       # q = pi
  np.testing.assert_allclose(np.delete(dq[0], n // 2), 0.0, atol=1e-14)
  _, at0 = lattice.dimer_structure_factor(bonds, pairs, connected, n, qs=[[0.0]])
  np.testing.assert_allclose(at0, 0.0, atol=1e-14)
  with pytest.raises(ValueError):
    lattice.dimer_structure_factor(bonds, pairs, connected[:-1], n)
  with pytest.raises(ValueError):
    lattice.dimer_structure_factor(bonds, [(0, n)], [0.0], n)
  with pytest.raises(ValueError):
    lattice.dimer_structure_factor([(0, n)], [(0, 0)], [0.0], n)


def test_file_readers_and_cli_lists(tmp_path):
  from cgs_vmc_amd import run_dimer_evaluation as rd
  f = tmp_path / 'bonds.txt'
  f.write_text('# bonds\n0 1\n\n2, 3   # another\n1 0\n0 1\n')
  bonds, pairs = lattice.read_bond_pairs(str(f))
  assert bonds == [[0, 1], [2, 3], [1, 0]] and pairs == []
  f.write_text('0 1 2 3\n2 3 0 1\n4 5\n0 1 0 1 # a == a\n')
  bonds, pairs = lattice.read_bond_pairs(str(f))
  assert bonds == [[0, 1], [2, 3], [4, 5]] and pairs == [[0, 1], [1, 0], [0, 0]]
  for bad in ('0 1 2\n', '0 x\n', '0 1 2 3 4\n', '0.5 1\n'):
    f.write_text('0 1\n' + bad)
    with pytest.raises(ValueError, match='bonds.txt:2'):
      lattice.read_bond_pairs(str(f))
  assert lattice.all_bond_pairs(3).tolist() == [[a, b] for a in range(3) for b in range(3)]
  assert lattice.all_bond_pairs(3).dtype == np.int32 and lattice.all_bond_pairs(0).shape == (0, 2)
  # the driver's lists: the Hamiltonian's bonds against the reference bond, or the file's
  b, p = rd.load_bond_pairs('', 2, BONDS8, N8)
  assert b.dtype == np.int32 and p.dtype == np.int32
  np.testing.assert_array_equal(b, BONDS8); np.testing.assert_array_equal(p, [(2, k) for k in range(N8)])
  f.write_text('0 1\n2 3\n4 5\n')
  b, p = rd.load_bond_pairs(str(f), 1, BONDS8, N8)
  np.testing.assert_array_equal(b, [(0, 1), (2, 3), (4, 5)]); np.testing.assert_array_equal(p, [(1, 0), (1, 1), (1, 2)])
  f.write_text('0 1 2 3\n2 3 2 3\n')
  b, p = rd.load_bond_pairs(str(f), 0, BONDS8, N8)
  np.testing.assert_array_equal(p, [(0, 1), (1, 1)])
  with pytest.raises(ValueError, match='reference_bond'):
    rd.load_bond_pairs('', N8, BONDS8, N8)
  f.write_text('0 8\n')
  with pytest.raises(ValueError, match='out of range'):
    rd.load_bond_pairs(str(f), 0, BONDS8, N8)
  f.write_text('3 3\n')
  with pytest.raises(ValueError, match='itself'):
    rd.load_bond_pairs(str(f), 0, BONDS8, N8)
  # the two files
  result = {'bonds': np.array(BONDS8, np.int32), 'pairs': np.array([(0, 0), (0, 3)], np.int32), 'dd': np.array([0.4, 0.1]),
            'dd_err': np.array([1e-3, 2e-3]), 'connected': np.array([0.2, -0.05]), 'connected_err': np.array([3e-3, 4e-3])}
  rows = np.loadtxt(rd.write_dimer_correlations(str(tmp_path), result))
  np.testing.assert_allclose(rows, [[0, 1, 0, 1, 0.4, 1e-3, 0.2, 3e-3], [0, 1, 3, 4, 0.1, 2e-3, -0.05, 4e-3]], rtol=1e-9)
  qs, dq = lattice.dimer_structure_factor(BONDS8, result['pairs'], result['connected'], N8)
  rows = np.loadtxt(rd.write_dimer_structure_factor(str(tmp_path), qs, dq))
  assert rows.shape == (N8, 2)
  np.testing.assert_allclose(rows[:, 0], qs[:, 0], rtol=1e-9); np.testing.assert_allclose(rows[:, 1], dq[0], rtol=1e-9, atol=1e-12)
  hp = types.SimpleNamespace(num_sites=N8, size_x=4, size_y=2)
  assert rd.lattice_sizes(hp, BONDS8) == (4, 2)
  hp = types.SimpleNamespace(num_sites=N8, size_x=0, size_y=0)
  assert rd.lattice_sizes(hp, BONDS8) == (N8, 1) and rd.lattice_sizes(hp, BONDS8[:-1]) is None

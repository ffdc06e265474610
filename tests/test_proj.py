"""CPU: the projected-energy estimator by full enumeration (tests/proj_oracle.py) against numpy.linalg.eigh,
lattice.sector_characters as projectors on the Sz = 0 space, lattice.check_hamiltonian_symmetry (the mirror of
plan_symm_check_hamiltonian, whose own cases run in csrc/hostcheck.cpp through tests/test_hostcheck.py),
ProjectedEnergyEvaluator's bookkeeping (ratio, jackknife, empty sectors, sharded sums) on a scripted engine double, the
characters file and the Python-side refusals."""
import types

import numpy as np
import pytest

from cgs_vmc_amd import evaluation
from cgs_vmc_amd import lattice
from cgs_vmc_amd import parallel
from cgs_vmc_amd import session as session_lib
from tests import edvec_oracle as eo
from tests import proj_oracle as pj
from tests import symm_oracle as so


def _flip_ops(size_x, size_y=1):
  t = lattice.translations(size_x, size_y)
  return np.concatenate([t, t]), np.repeat([0, 1], len(t)).astype(np.uint8)


@pytest.mark.parametrize('relative_sign', [1.0, -1.0])
def test_enumeration_of_the_mixture_gives_both_eigenvalues(relative_sign):
  """8-site chain, 0.95 v0 + sqrt(1 - 0.95^2) v1: sector (0, +) holds 0.9025 of the state at E0, (4, -) the rest at E1.
  The relative sign of the two vectors is immaterial: flipping it is the spin-flip image of the same state."""
  n = 8
  basis = eo.sz0_configurations(n)
  assert len(basis) == 70
  hmat = pj.hamiltonian_matrix(basis, lattice.chain_bonds(n), 1.0, 1.0)
  np.testing.assert_array_equal(hmat, hmat.T)
  w, v = np.linalg.eigh(hmat)
  state = 0.95 * v[:, 0] + relative_sign * np.sqrt(1.0 - 0.95 ** 2) * v[:, 1]
  perms, flips = _flip_ops(n)
  labels, chi = lattice.sector_characters(n, 1, True)
  weight, energy, plain = pj.exact_sectors(state, basis, hmat, perms, flips, chi)
  a, b = labels.index('q0+'), labels.index('q4-')
  assert abs(weight[a] - 0.9025) < 1e-12 and abs(weight[b] - 0.0975) < 1e-12
  assert abs(energy[a] - w[0]) < 1e-10 and abs(energy[b] - w[1]) < 1e-10
  others = np.ones(len(labels), bool); others[[a, b]] = False
  assert np.abs(weight[others]).max() < 1e-12
  assert abs(w[0] - (-3.651093)) < 1e-6 and abs(w[1] - (-3.128419)) < 1e-6 and abs(plain - (-3.600133)) < 1e-6
  # the sampled form of the same thing: chains = the whole basis weighted by |psi|^2 is what exact_sectors sums; the
  # per-chain oracle on the basis itself gives the same ratio once each chain is weighted by its probability
  psi = lambda c: state[pj.lookup(basis)(c)]
  eloc = (hmat @ state) / state
  wts, _, _ = pj.chain_weights(psi, basis, perms, flips, chi)
  p = state ** 2
  np.testing.assert_allclose((wts * p).sum(1), weight, atol=1e-13)
  np.testing.assert_allclose((wts[[a, b]] * eloc * p).sum(1) / (wts[[a, b]] * p).sum(1), w[:2], rtol=1e-11)


@pytest.mark.parametrize('size_x,size_y', [(6, 1), (4, 4)])
@pytest.mark.parametrize('spin_flip', [False, True])
def test_sector_characters_sum_to_the_identity_and_are_projectors(size_x, size_y, spin_flip):
  n = size_x * size_y
  labels, chi = lattice.sector_characters(size_x, size_y, spin_flip)
  classes = {(6, 1): 4, (4, 4): 10}[(size_x, size_y)]              # {k, -k} classes: (N + number of k = -k) / 2
  assert chi.shape == (classes * (2 if spin_flip else 1), n * (2 if spin_flip else 1))
  assert len(set(labels)) == len(labels) == len(chi) and all(len(l.split()) == 1 for l in labels)
  indicator = np.zeros(chi.shape[1]); indicator[0] = 1.0
  np.testing.assert_allclose(chi.sum(0), indicator, atol=1e-15)
  # the group algebra: chi_s * chi_t = delta_st chi_s under the convolution of the (abelian) group of the ops
  t = lattice.translations(size_x, size_y)
  table = np.array([[int(np.flatnonzero((t == t[a][t[b]]).all(1))[0]) for b in range(n)] for a in range(n)])   # T_a T_b
  if spin_flip:
    table = np.block([[table, table + n], [table + n, table]])
  for s in range(len(chi)):
    for u in range(len(chi)):
      conv = np.zeros(chi.shape[1])
      np.add.at(conv, table, np.outer(chi[s], chi[u]))
      np.testing.assert_allclose(conv, chi[s] if s == u else 0.0, atol=1e-15)
  if (size_x, size_y) != (6, 1):
    return
  # each P_s as a matrix on the Sz = 0 configuration space of the 6-site chain
  basis = eo.sz0_configurations(n)
  hmat = pj.hamiltonian_matrix(basis, lattice.chain_bonds(n), 1.0, 1.0)
  perms, flips = _flip_ops(n) if spin_flip else (t, None)
  ops = pj.op_matrices(basis, perms, flips)
  total = np.zeros_like(hmat)
  for row in chi:
    p = np.einsum('k,kxy->xy', row, ops)
    np.testing.assert_allclose(p @ p, p, atol=1e-14)
    np.testing.assert_allclose(p.T @ p, p, atol=1e-14)
    np.testing.assert_allclose(p @ hmat, hmat @ p, atol=1e-13)
    total += p
  np.testing.assert_allclose(total, np.eye(len(basis)), atol=1e-14)


def test_check_hamiltonian_symmetry():
  bonds = lattice.torus_bonds(4, 4, next_nearest=True)
  jx = np.array([1.0] * 32 + [0.5] * 32, np.float32)
  jz = np.array([1.0] * 32 + [0.25] * 32, np.float32)
  group = lattice.point_group(4, 4)[1]
  lattice.check_hamiltonian_symmetry(bonds, jx, jz, lattice.translations(4, 4))
  lattice.check_hamiltonian_symmetry(bonds, jx, jz, group)
  lattice.check_hamiltonian_symmetry(bonds, jx, jz, group[3])              # one op alone
  # the 2 x 4 torus names the bonds across its short direction twice: a multiset, not a set
  doubled = lattice.torus_bonds(2, 4)
  assert len(doubled) == 16 and len({(min(i, j), max(i, j)) for i, j in doubled}) == 12
  lattice.check_hamiltonian_symmetry(doubled, 1.0, 1.0, lattice.translations(2, 4))
  lattice.check_hamiltonian_symmetry(doubled, 1.0, 1.0, lattice.point_group(2, 4)[1])
  with pytest.raises(ValueError, match='op 2 is no symmetry'):
    lattice.check_hamiltonian_symmetry(doubled[1:], 1.0, 1.0, lattice.translations(2, 4))    # T(0,1) misses the dropped twin
  rand = np.random.default_rng(12).permutation(16)
  with pytest.raises(ValueError, match=r'op 1 is no symmetry of the Hamiltonian: bond \d+ = \(\d+, \d+\) goes to'):
    lattice.check_hamiltonian_symmetry(bonds, jx, jz, np.stack([np.arange(16), rand]))
  # one bond's j_x changed: T(1,0) maps bond 2 = (1, 2) onto (2, 3), which carries another coupling
  changed = jx.copy(); changed[4] = 0.75                                   # bond 4 = (2, 3)
  assert tuple(bonds[4]) == (2, 3) and tuple(bonds[2]) == (1, 2)
  lattice.check_hamiltonian_symmetry(bonds, changed, jz, lattice.translations(4, 4)[0])
  with pytest.raises(ValueError, match=r'op 1 is no symmetry of the Hamiltonian: bond 2 = \(1, 2\) goes to \(2, 3\)'):
    lattice.check_hamiltonian_symmetry(bonds, changed, jz, lattice.translations(4, 4))
  # the couplings are compared as the float32 the library holds
  lattice.check_hamiltonian_symmetry(lattice.chain_bonds(8), 1.0 + 1e-12, 1.0, lattice.translations(8))
  with pytest.raises(ValueError):
    lattice.check_hamiltonian_symmetry([], 1.0, 1.0, lattice.translations(8))


class _ScriptedEngine:
  """Engine double: projected_energy returns the next scripted dict; run_many counts the sampler's calls."""

  def __init__(self, script):
    self.script, self.at, self.steps = list(script), 0, []

  def projected_energy(self, perms, flips, characters, which=0, ops_per_pass=0):
    assert which == 0 and ops_per_pass == 0
    out = self.script[self.at]
    self.at += 1
    return out

  def run_many(self, n):
    self.steps.append(n)


N8 = 8
OPS8 = _flip_ops(N8)
CHI8 = lattice.sector_characters(N8, 1, True)[1]


def _script(n_samples, n_sectors, seed, batch):
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(n_samples):
    w = rng.uniform(0.2, 1.0, n_sectors) * batch
    w[3] = 0.0                                            # a sector the state has exactly no weight in
    out.append({'w_sum': w, 'we_sum': w * rng.uniform(-3.7, -3.1, n_sectors), 'e_sum': -3.5 * batch + rng.standard_normal(),
                'n_alive': batch - int(rng.integers(0, 3))})
  return out


def _ops(engine, ensure=None):
  mc = session_lib.Op(lambda: None, 'mc_step')
  mc.last_accepted = 3
  mc.run_many = engine.run_many
  value = evaluation.ProjectedEnergyTensor(engine, OPS8[0], OPS8[1], CHI8, 0, N8, ensure)
  return evaluation.EvalOps(value=value, mc_step=mc, acceptance_rate=None, placeholder_input=None, wavefunction_value=None)


def _hparams(n_samples, batch, **kw):
  return types.SimpleNamespace(num_sites=N8, batch_size=batch, num_equilibration_sweeps=5, num_monte_carlo_sweeps=2,
                               num_evaluation_samples=n_samples, **kw)


def test_evaluator_ratio_jackknife_and_empty_sectors():
  n_samples, batch, n_s = 7, 64, len(CHI8)
  script = _script(n_samples, n_s, 1, batch)
  ensured = []
  eng = _ScriptedEngine(script)
  ev = evaluation.ProjectedEnergyEvaluator()
  out = ev.run_evaluation(_ops(eng, lambda: ensured.append(1)), session_lib.Session(), _hparams(n_samples, batch), epoch_num=0)
  assert set(out) == {'perms', 'flips', 'characters', 'energy', 'energy_err', 'weight', 'weight_err', 'plain_energy',
                      'plain_energy_err', 'samples'}
  assert eng.at == n_samples == len(ensured) and eng.steps == [5 * N8] + [2 * N8] * n_samples
  assert ev.acceptance_count == 3 * n_samples
  w = np.array([s['w_sum'] for s in script]); we = np.array([s['we_sum'] for s in script])
  e = np.array([s['e_sum'] for s in script]); alive = np.array([s['n_alive'] for s in script], np.float64)
  np.testing.assert_array_equal(out['samples'], np.concatenate([w, we, e[:, None], alive[:, None]], axis=1))
  live = np.arange(n_s) != 3
  np.testing.assert_allclose(out['energy'][live], we.sum(0)[live] / w.sum(0)[live], rtol=1e-15)
  # the delete-one jackknife, by hand
  theta = np.array([(we.sum(0) - we[t])[live] / (w.sum(0) - w[t])[live] for t in range(n_samples)])
  err = np.sqrt((n_samples - 1) / n_samples * ((theta - theta.mean(0)) ** 2).sum(0))
  np.testing.assert_allclose(out['energy_err'][live], err, rtol=1e-12)
  assert np.isnan(out['energy'][3]) and np.isnan(out['energy_err'][3])              # nan, never an exception
  assert out['weight'][3] == 0.0 and out['weight_err'][3] == 0.0
  np.testing.assert_allclose(out['weight'], w.sum(0) / alive.sum(), rtol=1e-15)
  np.testing.assert_allclose(out['weight_err'], (w / alive[:, None]).std(0, ddof=1) / np.sqrt(n_samples), rtol=1e-13)
  assert abs(out['plain_energy'] - e.sum() / alive.sum()) < 1e-14
  assert abs(out['plain_energy_err'] - (e / alive).std(ddof=1) / np.sqrt(n_samples)) < 1e-15
  # a single sample has no spread to report
  one = evaluation.ProjectedEnergyEvaluator().run_evaluation(
      _ops(_ScriptedEngine(script[:1])), session_lib.Session(), _hparams(1, batch), epoch_num=0)
  assert (one['energy_err'][live] == 0).all() and (one['weight_err'] == 0).all() and one['plain_energy_err'] == 0
  np.testing.assert_allclose(one['energy'][live], we[0][live] / w[0][live], rtol=1e-15)
  assert np.isnan(one['energy'][3])


def test_evaluator_two_ranks_of_scripted_shards_give_the_unsharded_result(monkeypatch):
  n_samples, batch, n_s = 4, 32, len(CHI8)
  mine, theirs = _script(n_samples, n_s, 2, batch), _script(n_samples, n_s, 3, batch)
  stack = lambda s: np.concatenate([s['w_sum'], s['we_sum'], [s['e_sum'], s['n_alive']]])
  reduced = []

  def fake_allreduce(values, op='sum'):
    values = np.asarray(values)
    assert op == 'sum' and values.dtype == np.float64 and values.shape == (2 * n_s + 2,)
    reduced.append(values.copy())
    return values + stack(theirs[len(reduced) - 1])
  monkeypatch.setattr(parallel, 'world_size', lambda: 2)
  monkeypatch.setattr(parallel, 'allreduce_array', fake_allreduce)
  sharded = evaluation.ProjectedEnergyEvaluator().run_evaluation(
      _ops(_ScriptedEngine(mine)), session_lib.Session(), _hparams(n_samples, 2 * batch), epoch_num=0)
  assert len(reduced) == n_samples                      # one collective per sample, on the stacked fp64 sums
  for s in range(n_samples):
    np.testing.assert_array_equal(reduced[s], stack(mine[s]))
  monkeypatch.setattr(parallel, 'world_size', lambda: 1)
  reduced.clear()
  whole = [{'w_sum': a['w_sum'] + b['w_sum'], 'we_sum': a['we_sum'] + b['we_sum'], 'e_sum': a['e_sum'] + b['e_sum'],
            'n_alive': a['n_alive'] + b['n_alive']} for a, b in zip(mine, theirs)]
  single = evaluation.ProjectedEnergyEvaluator().run_evaluation(
      _ops(_ScriptedEngine(whole)), session_lib.Session(), _hparams(n_samples, 2 * batch), epoch_num=0)
  assert reduced == []                                  # single rank: no collective at all
  for key in ('energy', 'energy_err', 'weight', 'weight_err', 'plain_energy', 'plain_energy_err', 'samples'):
    np.testing.assert_array_equal(sharded[key], single[key])


def test_evaluator_default_sectors_and_python_side_refusals(monkeypatch):
  eng = _ScriptedEngine([])
  wf = types.SimpleNamespace(_which=0, _bind=lambda configs: eng)
  monkeypatch.setattr(evaluation.graph_builders, 'get_configs', lambda *a, **k: None)
  monkeypatch.setattr(evaluation.graph_builders, 'get_monte_carlo_sampling', lambda *a, **k: (None, None))
  build = lambda operator, **sizes: evaluation.ProjectedEnergyEvaluator().build_eval_ops(wf, operator, _hparams(1, 16, **sizes), {})
  ops = build((None, None, None, None), size_x=4, size_y=2)
  np.testing.assert_array_equal(ops.value.perms, lattice.translations(4, 2))
  np.testing.assert_array_equal(ops.value.characters, lattice.sector_characters(4, 2)[1])
  assert not ops.value.flips.any()
  for sizes in (dict(size_x=3, size_y=2), dict()):
    with pytest.raises(ValueError, match='size_x'):
      build((None, None, None, None), **sizes)
  # refused before any library call: the double would raise IndexError if it were asked
  with pytest.raises(ValueError, match='op 0'):
    build((None, [[0] * N8], None, [[1.0]]))
  with pytest.raises(ValueError, match='characters'):
    build((None, OPS8[0], OPS8[1], CHI8[:, :5]))
  bad = CHI8.copy(); bad[2, 4] = np.inf
  with pytest.raises(ValueError, match='sector 2: the character of op 4'):
    build((None, OPS8[0], OPS8[1], bad))
  for chi in (np.zeros((0, 16)), [], 'abc', np.zeros((2, 2, 16))):
    with pytest.raises(ValueError):
      lattice.check_characters(chi, 16)
  assert lattice.check_characters(np.ones(16), 16).shape == (1, 16)          # one row alone is one sector
  with pytest.raises(ValueError):
    lattice.sector_characters(0, 1)

  class _NoLibrary:
    n_sites = N8

    def __getattr__(self, name):
      raise AssertionError('the library was reached: ' + name)
  from cgs_vmc_amd.engine import VmcEngine
  for args in ((OPS8[0][:, :7], OPS8[1], CHI8), (OPS8[0], OPS8[1], bad), (OPS8[0], OPS8[1][:3], CHI8),
               (OPS8[0], OPS8[1], CHI8[:, :3])):
    with pytest.raises(ValueError):
      VmcEngine.projected_energy(_NoLibrary(), *args)


def test_characters_file_round_trip(tmp_path):
  labels, chi = lattice.sector_characters(4, 4, True)
  path = str(tmp_path / 'chi.txt')
  lattice.write_characters(path, labels, chi)
  back_labels, back = lattice.read_characters(path)
  assert back_labels == labels
  np.testing.assert_array_equal(back, chi)                                  # 17 digits: the same bits
  with open(path, 'a') as f:
    f.write('\n# a comment\nextra ' + '  '.join(['0.5'] * chi.shape[1]) + '   # a trailing comment\n')
  back_labels, back = lattice.read_characters(path)
  assert back_labels == labels + ['extra'] and (back[-1] == 0.5).all()
  for text in ('q0 1.0 2.0\nq1 1.0\n', 'q0 1.0 nan\n', 'q0 1.0 x\n', 'q0\n', '# nothing\n'):
    bad = str(tmp_path / 'bad.txt')
    with open(bad, 'w') as f:
      f.write(text)
    with pytest.raises(ValueError):
      lattice.read_characters(bad)
  with pytest.raises(ValueError):
    lattice.write_characters(path, ['a b'], [[1.0]])
  with pytest.raises(ValueError):
    lattice.write_characters(path, ['a'], [[1.0], [2.0]])


def test_driver_default_sectors_and_file(tmp_path):
  from cgs_vmc_amd import run_projected_energy_evaluation as rp
  hp = types.SimpleNamespace(num_sites=8, size_x=0, size_y=0)
  labels, perms, flips, chi = rp.load_sectors('', '', True, hp, lattice.chain_bonds(8))
  assert labels == lattice.sector_characters(8, 1, True)[0] and chi.shape == (10, 16)
  np.testing.assert_array_equal(perms, OPS8[0]); np.testing.assert_array_equal(flips, OPS8[1])
  labels, perms, flips, chi = rp.load_sectors('', '', False, hp, lattice.chain_bonds(8))
  assert chi.shape == (5, 8) and not flips.any()
  with pytest.raises(ValueError, match='go together'):
    rp.load_sectors('ops.txt', '', False, hp, lattice.chain_bonds(8))
  ops_path, chi_path = str(tmp_path / 'ops.txt'), str(tmp_path / 'chi.txt')
  lattice.write_symmetry_ops(ops_path, OPS8[0][[0, 8]], OPS8[1][[0, 8]])
  lattice.write_characters(chi_path, ['even', 'odd'], [[0.5, 0.5], [0.5, -0.5]])
  labels, perms, flips, chi = rp.load_sectors(ops_path, chi_path, False, hp, lattice.chain_bonds(8))
  assert labels == ['even', 'odd'] and flips.tolist() == [0, 1] and chi.tolist() == [[0.5, 0.5], [0.5, -0.5]]
  result = {'weight': np.array([0.9, 0.001, 0.0]), 'weight_err': np.array([0.01, 0.002, 0.0]),
            'energy': np.array([-3.65, -1.0, np.nan]), 'energy_err': np.array([0.002, 5.0, np.nan]),
            'plain_energy': -3.6, 'plain_energy_err': 0.001}
  path = rp.write_sector_energies(str(tmp_path), ['a', 'b', 'c'], result)
  lines = [l.split() for l in open(path) if not l.startswith('#')]
  assert [l[0] for l in lines] == ['a', 'b', 'c'] and [len(l) for l in lines] == [5, 6, 5] and lines[1][5] == 'unresolved'
  assert float(lines[0][3]) == -3.65 and lines[2][3] == 'nan'

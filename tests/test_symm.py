"""CPU: the symmetry oracle against itself, lattice.translations / point_group / check_symmetry_ops / read_symmetry_ops /
momentum_weights against exact characters of Heisenberg ground states, SymmetryEvaluator's bookkeeping (errors, sharded
sums) on an engine double that gets symmetry_expectations from the oracle, and the helpers of run_symmetry_evaluation."""
import functools
import types

import numpy as np
import pytest

from cgs_vmc_amd import evaluation
from cgs_vmc_amd import lattice
from cgs_vmc_amd import parallel
from cgs_vmc_amd import session as session_lib
from tests import edvec_oracle as eo
from tests import exact_states
from tests import symm_oracle as so

N6 = 6


@functools.lru_cache(maxsize=None)
def _chain6(jx):
  """(vector in Lin order, index(configs), basis) of the 6-site chain's ground state at j_x = jx."""
  _, vec, cfgs, _ = exact_states.ed_ground_state(N6, lattice.chain_bonds(N6), jx, 1.0)
  top, bot, length = eo.lin_tables(N6)
  out = np.zeros(length)
  out[eo.index(cfgs, top, bot)] = vec
  return out, (lambda c: eo.index(c, top, bot)), eo.sz0_configurations(N6)


def _random_psi(n, seed, zeros=0):
  rng = np.random.default_rng(seed)
  top, bot, length = eo.lin_tables(n)
  vec = rng.standard_normal(length)
  if zeros:
    vec[rng.integers(0, length, zeros)] = 0.0
  return vec, (lambda c: eo.amplitude(vec, c, top, bot))


def test_oracle_identity_gives_the_batch_and_an_op_undoes_its_inverse():
  rng = np.random.default_rng(0)
  n, b = 8, 30
  _, psi = _random_psi(n, 1)
  cfg = eo.sz0_configurations(n)[rng.permutation(70)[:b]]
  ident = np.arange(n)
  np.testing.assert_array_equal(so.rows(cfg, ident, 0), cfg)
  np.testing.assert_array_equal(so.rows(cfg, ident, 1), -cfg)
  assert so.sums(psi, cfg, [ident])[0] == b
  for flip in (0, 1):
    g = rng.permutation(n)
    inv = np.argsort(g)
    moved = so.rows(cfg, g, flip)
    np.testing.assert_array_equal(so.rows(moved, inv, flip), cfg)         # g^-1 at the permuted rows is x again
    t = so.terms(psi, cfg, [g], [flip])[0]
    t_back = so.terms(psi, moved, [inv], [flip])[0]
    np.testing.assert_allclose(t * t_back, 1.0, rtol=1e-14)
  # a vanishing amplitude on either side gives exactly 0, never NaN
  vec0, psi0 = _random_psi(n, 2, zeros=25)
  ops = [rng.permutation(n) for _ in range(4)]
  t = so.terms(psi0, cfg, ops, [0, 1, 0, 1])
  assert np.isfinite(t).all()
  dead = psi0(cfg) == 0
  assert dead.any() and (t[:, dead] == 0).all()
  for k, (g, f) in enumerate(zip(ops, [0, 1, 0, 1])):
    assert (t[k, psi0(so.rows(cfg, g, f)) == 0] == 0).all()
  np.testing.assert_allclose(so.sums(psi0, cfg, ops, [0, 1, 0, 1]), t.sum(1), rtol=1e-15)


@pytest.mark.parametrize('size_x,size_y', [(6, 1), (4, 4), (4, 3), (3, 5)])
def test_translations_and_point_group_are_bijections_that_compose(size_x, size_y):
  n = size_x * size_y
  t = lattice.translations(size_x, size_y)
  assert t.shape == (n, n) and t.dtype == np.int32
  np.testing.assert_array_equal(t[0], np.arange(n))
  for g in t:
    np.testing.assert_array_equal(np.sort(g), np.arange(n))
  # row = s[perm]: applying T_a and then T_b gathers through perm_a[perm_b]
  for a in range(n):
    for b in range(n):
      ab = (a % size_x + b % size_x) % size_x + size_x * ((a // size_x + b // size_x) % size_y)
      np.testing.assert_array_equal(t[a][t[b]], t[ab])
  labels, group = lattice.point_group(size_x, size_y)
  assert labels[0] == 'identity' and group.dtype == np.int32 and group.shape == (len(labels), n)
  np.testing.assert_array_equal(group[0], np.arange(n))
  assert len(labels) == (2 if size_y == 1 else 8 if size_x == size_y else 4)
  assert len({tuple(g) for g in group.tolist()}) == len(labels) == len(set(labels))
  for g in group:
    np.testing.assert_array_equal(np.sort(g), np.arange(n))
    assert g[0] == 0                                                     # about site 0
  # closed under composition (the eight square ops are C4v, not abelian)
  members = {tuple(g) for g in group.tolist()}
  for g in group:
    for h in group:
      assert tuple(g[h].tolist()) in members
  if size_x == size_y:
    rot, mx = group[labels.index('rot90')], group[labels.index('mirror_x')]
    np.testing.assert_array_equal(rot[rot], group[labels.index('rot180')])
    np.testing.assert_array_equal(rot[rot][rot], group[labels.index('rot270')])
    assert not np.array_equal(rot[mx], mx[rot])
  # every op maps bonds of the lattice to bonds of the lattice
  bonds = lattice.chain_bonds(n) if size_y == 1 else lattice.torus_bonds(size_x, size_y)
  as_set = {(min(i, j), max(i, j)) for i, j in bonds}
  for g in list(t) + list(group):
    inv = np.argsort(g)
    assert {(min(inv[i], inv[j]), max(inv[i], inv[j])) for i, j in as_set} == as_set


def test_check_symmetry_ops_and_the_ops_file(tmp_path):
  n = 6
  good = [[1, 2, 3, 4, 5, 0], [0, 5, 4, 3, 2, 1]]
  p, f = lattice.check_symmetry_ops(good, None, n)
  assert p.dtype == np.int32 and p.shape == (2, n) and p.flags['C_CONTIGUOUS']
  assert f.dtype == np.uint8 and f.tolist() == [0, 0]
  p, f = lattice.check_symmetry_ops(np.asarray(good, np.int64)[:, ::1], [True, False], n)
  assert f.tolist() == [1, 0]
  p1, f1 = lattice.check_symmetry_ops(good[0], [1], n)                    # one op alone
  assert p1.shape == (1, n) and f1.tolist() == [1]
  with pytest.raises(ValueError, match='op 1'):
    lattice.check_symmetry_ops([good[0], [0, 5, 4, 3, 2, 2]], None, n)    # a duplicate
  with pytest.raises(ValueError, match='op 1.*entry 5'):
    lattice.check_symmetry_ops([good[0], [0, 5, 4, 3, 2, n]], None, n)    # a site out of range
  with pytest.raises(ValueError, match='op 0'):
    lattice.check_symmetry_ops([[-1, 2, 3, 4, 5, 0]], None, n)
  with pytest.raises(ValueError):
    lattice.check_symmetry_ops([[0, 1, 2, 3, 4]], None, n)                # a wrong length
  with pytest.raises(ValueError):
    lattice.check_symmetry_ops([[0, 1, 2, 3, 4, 5, 6]], None, n)
  with pytest.raises(ValueError, match='op 1.*flip'):
    lattice.check_symmetry_ops(good, [0, 2], n)                           # a flip of 2
  with pytest.raises(ValueError):
    lattice.check_symmetry_ops(good, [0], n)
  with pytest.raises(ValueError):
    lattice.check_symmetry_ops(good, [0.5, 0.5], n)
  with pytest.raises(ValueError):
    lattice.check_symmetry_ops([], None, n)                               # no ops
  with pytest.raises(ValueError):
    lattice.check_symmetry_ops(np.zeros((0, n), np.int32), None, n)
  with pytest.raises(ValueError):
    lattice.check_symmetry_ops([[0.5, 1, 2, 3, 4, 5]], None, n)
  # the file: written, read back, comments and blank lines skipped
  path = str(tmp_path / 'ops.txt')
  lattice.write_symmetry_ops(path, good, [0, 1], labels=['T(1)', 'mirror+flip'])
  perms, flips = lattice.read_symmetry_ops(path)
  assert perms == good and flips == [0, 1]
  (tmp_path / 'ops2.txt').write_text('# ops\n1 2 3 4 5 0\n\nflip 0, 5, 4 3 2 1   # mirror, then the flip\nFLIP 0 1 2 3 4 5\n')
  perms, flips = lattice.read_symmetry_ops(str(tmp_path / 'ops2.txt'))
  assert perms == good + [[0, 1, 2, 3, 4, 5]] and flips == [0, 1, 1]
  (tmp_path / 'bad.txt').write_text('0 1 2\nflip\n')
  with pytest.raises(ValueError, match='bad.txt:2'):
    lattice.read_symmetry_ops(str(tmp_path / 'bad.txt'))
  (tmp_path / 'bad.txt').write_text('0 1 x\n')
  with pytest.raises(ValueError, match='bad.txt:1'):
    lattice.read_symmetry_ops(str(tmp_path / 'bad.txt'))


def test_momentum_weights_and_exact_characters_on_the_6_site_chain():
  plus, index, basis = _chain6(1.0)
  minus, _, _ = _chain6(-1.0)
  t = lattice.translations(N6)
  _, group = lattice.point_group(N6)
  ident = np.arange(N6)
  # the characters the GPU tests use: j_x = +1 has momentum pi, an even mirror and odd spin inversion
  for perm, flip, want in ((t[1], 0, -1.0), (t[2], 0, 1.0), (group[1], 0, 1.0), (ident, 1, -1.0), (ident, 0, 1.0)):
    assert abs(so.exact_expectation(plus, basis, index, perm, flip) - want) < 1e-12
  mix = 0.6 * minus + 0.8 * plus                       # k = 0 and k = pi: orthogonal, whatever signs eigsh picked
  values = np.array([so.exact_expectation(mix, basis, index, t[r], 0) for r in range(N6)])
  np.testing.assert_allclose(values, [1, -0.28, 1, -0.28, 1, -0.28], atol=1e-12)
  w = lattice.momentum_weights(values, N6)
  np.testing.assert_allclose(w, [0.36, 0, 0, 0.64, 0, 0], atol=1e-12)
  assert abs(w.sum() - values[0]) < 1e-12
  np.testing.assert_allclose(lattice.chain_momenta(N6)[3], [np.pi])
  # leading axes are samples; the transform is linear
  stack = np.stack([values, 2 * values, np.ones(N6)])
  ws = lattice.momentum_weights(stack, N6)
  assert ws.shape == (3, N6)
  np.testing.assert_allclose(ws[1], 2 * w, atol=1e-12)
  np.testing.assert_allclose(ws[2], [1, 0, 0, 0, 0, 0], atol=1e-12)
  with pytest.raises(ValueError):
    lattice.momentum_weights(values[:5], N6)
  # a torus: a plane wave cos(q . r) has the weight 1/2 at q and at -q
  sx, sy = 4, 3
  qs = lattice.torus_momenta(sx, sy)
  r = lattice.torus_coords(sx, sy)
  m = 1 + sx * 2                                       # q = (2 pi / 4, 4 pi / 3); -q is m_x = 3, m_y = 1
  w2 = lattice.momentum_weights(np.cos(r @ qs[m]), sx, sy)
  want = np.zeros(sx * sy); want[m] = 0.5; want[3 + sx * 1] = 0.5
  np.testing.assert_allclose(w2, want, atol=1e-12)


def test_exact_characters_of_the_4x4_ground_states_are_all_one():
  bonds = sorted({(min(i, j), max(i, j)) for i, j in lattice.torus_bonds(4, 4)})
  top, bot, length = eo.lin_tables(16)
  basis = eo.sz0_configurations(16)
  index = lambda c: eo.index(c, top, bot)
  ops = list(lattice.translations(4, 4)) + list(lattice.point_group(4, 4)[1])
  for jx in (1.0, -1.0):
    _, vec, _, _ = eo.vector_from_ed(16, bonds, jx, 1.0)
    for perm in ops:
      assert abs(so.exact_expectation(vec, basis, index, perm, 0) - 1.0) < 1e-9
    assert abs(so.exact_expectation(vec, basis, index, np.arange(16), 1) - 1.0) < 1e-9


class _OracleEngine:
  """Engine double: a scripted list of chain sets; symmetry_expectations is the oracle's on the current set, mc_steps
  (run_many of the sampler op) moves on to the next set after the thermalisation call."""

  def __init__(self, psi, chain_sets):
    self.psi, self.sets, self.at, self.steps, self.calls = psi, list(chain_sets), 0, [], 0
    self.batch_size = len(self.sets[0])

  def symmetry_expectations(self, perms, flips=None, which=0, ops_per_pass=0):
    assert which == 0 and ops_per_pass == 0
    self.calls += 1
    return so.sums(self.psi, self.sets[self.at], perms, flips)

  def run_many(self, n):
    if self.steps:                                        # (the first call is the thermalisation)
      self.at = min(self.at + 1, len(self.sets) - 1)
    self.steps.append(n)


N8 = 8
OPS8 = (np.concatenate([lattice.translations(N8), lattice.point_group(N8)[1][1:], np.arange(N8)[None, :]]),
        np.array([0] * 9 + [1], np.uint8))


def _ops(engine, operator, global_batch):
  mc = session_lib.Op(lambda: None, 'mc_step')
  mc.last_accepted = 3
  mc.run_many = engine.run_many
  value = evaluation.SymmetryTensor(engine, operator[0], operator[1], 0, N8, global_batch)
  return evaluation.EvalOps(value=value, mc_step=mc, acceptance_rate=None, placeholder_input=None, wavefunction_value=None)


def _hparams(n_samples, batch, **kw):
  return types.SimpleNamespace(num_sites=N8, batch_size=batch, num_equilibration_sweeps=5, num_monte_carlo_sweeps=2,
                               num_evaluation_samples=n_samples, **kw)


def _chain_sets(n_sets, batch, seed):
  rng = np.random.default_rng(seed)
  basis = eo.sz0_configurations(N8)
  return [basis[rng.integers(0, len(basis), batch)] for _ in range(n_sets)]


def test_evaluator_dict_and_standard_errors_on_the_oracle_double(monkeypatch):
  _, psi = _random_psi(N8, 3)
  n_samples, batch = 6, 24
  sets = _chain_sets(n_samples, batch, 1)
  eng = _OracleEngine(psi, sets)
  ev = evaluation.SymmetryEvaluator()
  out = ev.run_evaluation(_ops(eng, OPS8, batch), session_lib.Session(), _hparams(n_samples, batch), epoch_num=0)
  assert set(out) == {'perms', 'flips', 'value', 'value_err', 'samples'}
  assert eng.calls == n_samples and eng.steps == [5 * N8] + [2 * N8] * n_samples
  assert ev.acceptance_count == 3 * n_samples
  np.testing.assert_array_equal(out['perms'], OPS8[0]); np.testing.assert_array_equal(out['flips'], OPS8[1])
  assert out['perms'].dtype == np.int32 and out['flips'].dtype == np.uint8
  ref = np.array([so.sums(psi, s, *OPS8) / batch for s in sets])
  np.testing.assert_allclose(out['samples'], ref, rtol=1e-15)
  np.testing.assert_allclose(out['value'], ref.mean(0), rtol=1e-14)
  err = np.sqrt(((ref - ref.mean(0)) ** 2).sum(0) / (n_samples - 1) / n_samples)          # per op, by hand
  np.testing.assert_allclose(out['value_err'], err, rtol=1e-13, atol=1e-17)
  assert out['value'][0] == 1.0 and out['value_err'][0] == 0.0                            # the identity
  # a single sample has no spread to report
  one = evaluation.SymmetryEvaluator().run_evaluation(
      _ops(_OracleEngine(psi, sets[:1]), OPS8, batch), session_lib.Session(), _hparams(1, batch), epoch_num=0)
  assert (one['value_err'] == 0).all() and one['samples'].shape == (1, 10)
  np.testing.assert_allclose(one['value'], ref[0], rtol=1e-15)
  # operator = None means the translations of size_x x size_y, when they fit num_sites
  wf = types.SimpleNamespace(_which=0, _bind=lambda configs: eng)
  monkeypatch.setattr(evaluation.graph_builders, 'get_configs', lambda *a, **k: None)
  monkeypatch.setattr(evaluation.graph_builders, 'get_monte_carlo_sampling', lambda *a, **k: (None, None))
  ops = evaluation.SymmetryEvaluator().build_eval_ops(wf, None, _hparams(1, batch, size_x=4, size_y=2), {})
  np.testing.assert_array_equal(ops.value.perms, lattice.translations(4, 2))
  assert not ops.value.flips.any() and ops.value.global_batch == batch
  for sizes in (dict(size_x=1, size_y=1), dict(size_x=3, size_y=2), dict()):
    with pytest.raises(ValueError, match='size_x'):
      evaluation.SymmetryEvaluator().build_eval_ops(wf, None, _hparams(1, batch, **sizes), {})
  with pytest.raises(ValueError, match='op 0'):
    evaluation.SymmetryEvaluator().build_eval_ops(wf, ([[0] * N8], None), _hparams(1, batch), {})


def test_evaluator_adds_sharded_sums_before_the_division_by_the_global_batch(monkeypatch):
  _, psi = _random_psi(N8, 4)
  n_samples, local_batch, world = 3, 16, 2
  sets = _chain_sets(n_samples, local_batch, 2)
  other = np.linspace(1.0, 2.0, 10)                      # what the second rank adds to every sample
  reduced = []

  def fake_allreduce(values, op='sum'):
    values = np.asarray(values)
    assert op == 'sum' and values.dtype == np.float64 and values.shape == (10,)
    reduced.append(values.copy())
    return values + other
  monkeypatch.setattr(parallel, 'world_size', lambda: world)
  monkeypatch.setattr(parallel, 'allreduce_array', fake_allreduce)
  out = evaluation.SymmetryEvaluator().run_evaluation(
      _ops(_OracleEngine(psi, sets), OPS8, world * local_batch), session_lib.Session(),
      _hparams(n_samples, world * local_batch), epoch_num=0)
  assert len(reduced) == n_samples                      # one collective per sample, on the fp64 sums
  for s in range(n_samples):
    mine = so.sums(psi, sets[s], *OPS8)
    np.testing.assert_array_equal(reduced[s], mine)
    np.testing.assert_allclose(out['samples'][s], (mine + other) / (world * local_batch), rtol=1e-15)
  # single rank: no collective at all
  reduced.clear()
  monkeypatch.setattr(parallel, 'world_size', lambda: 1)
  evaluation.SymmetryEvaluator().run_evaluation(
      _ops(_OracleEngine(psi, sets), OPS8, local_batch), session_lib.Session(), _hparams(n_samples, local_batch), epoch_num=0)
  assert reduced == []


def test_driver_default_ops_labels_and_files(tmp_path):
  from cgs_vmc_amd import run_symmetry_evaluation as rs
  labels, perms, flips = rs.default_ops(6, 1, False)
  assert labels == ['T(%d)' % r for r in range(6)] + ['mirror']
  np.testing.assert_array_equal(perms[:6], lattice.translations(6)); assert not flips.any()
  labels, perms, flips = rs.default_ops(4, 4, True)
  assert len(labels) == len(perms) == len(flips) == 2 * (16 + 7) and len(set(labels)) == len(labels)
  assert labels[1] == 'T(1,0)' and labels[4] == 'T(0,1)' and labels[16] == 'rot90' and labels[23] == 'flip'
  assert labels[24] == 'T(1,0)+flip' and labels[-1] == 'mirror_antidiag+flip'
  np.testing.assert_array_equal(perms[23], np.arange(16)); np.testing.assert_array_equal(perms[23:], perms[:23])
  assert flips.tolist() == [0] * 23 + [1] * 23
  assert all(' ' not in name for name in labels)
  lattice.check_symmetry_ops(perms, flips, 16)
  # load_ops: the geometry from hparams or from the chain's bonds, else an ops file
  hp = types.SimpleNamespace(num_sites=6, size_x=1, size_y=1)
  assert rs.lattice_sizes(hp, lattice.chain_bonds(6)) == (6, 1)
  assert rs.lattice_sizes(types.SimpleNamespace(num_sites=6, size_x=3, size_y=2), []) == (3, 2)
  assert rs.lattice_sizes(hp, [(0, 3)]) is None
  with pytest.raises(ValueError, match='ops_file'):
    rs.load_ops('', False, hp, [(0, 3)])
  names, p, f = rs.load_ops('', True, hp, lattice.chain_bonds(6))
  assert len(names) == 14 and p.shape == (14, 6) and f.sum() == 7
  path = str(tmp_path / 'ops.txt')
  lattice.write_symmetry_ops(path, p[[1, 6]], [0, 1])
  names, p2, f2 = rs.load_ops(path, False, hp, [(0, 3)])
  assert names == ['op0', 'op1'] and f2.tolist() == [0, 1]
  np.testing.assert_array_equal(p2, p[[1, 6]])
  (tmp_path / 'short.txt').write_text('0 1 2\n')
  with pytest.raises(ValueError, match='6 site indices'):
    rs.load_ops(str(tmp_path / 'short.txt'), False, hp, [])
  (tmp_path / 'twice.txt').write_text('0 1 2 3 4 4\n')
  with pytest.raises(ValueError, match='op 0'):
    rs.load_ops(str(tmp_path / 'twice.txt'), False, hp, [])
  # the two files from a canned result: the mixture 0.36 at q = 0, 0.64 at q = pi, two samples around it
  labels, perms, flips = rs.default_ops(6, 1, True)
  base = np.concatenate([[1, -0.28, 1, -0.28, 1, -0.28], [0.5], [-1] * 7])
  wiggle = np.zeros(14); wiggle[1] = 0.06
  samples = np.stack([base + wiggle, base - wiggle])
  result = {'perms': perms, 'flips': flips, 'value': samples.mean(0), 'value_err': evaluation._std_err(samples),
            'samples': samples}
  written = rs.write_files(str(tmp_path), hp, lattice.chain_bonds(6), labels, result)
  assert [w.rsplit('/', 1)[1] for w in written] == ['symmetries.txt', 'momentum_weights.txt']
  lines = [l.split() for l in open(written[0]) if not l.startswith('#')]
  assert [l[0] for l in lines] == labels and [int(l[1]) for l in lines] == flips.tolist()
  np.testing.assert_allclose([float(l[2]) for l in lines], base, rtol=1e-9)
  np.testing.assert_allclose([float(l[3]) for l in lines], result['value_err'], rtol=1e-2)
  rows = np.loadtxt(written[1])
  assert rows.shape == (6, 3)
  np.testing.assert_allclose(rows[:, 0], lattice.chain_momenta(6)[:, 0], rtol=1e-9)
  np.testing.assert_allclose(rows[:, 1], [0.36, 0, 0, 0.64, 0, 0], atol=1e-9)
  # the error of a weight is that of the per-sample weights: w[m] moves by cos(q_m) 0.06 / 6 either way
  np.testing.assert_allclose(rows[:, 2], np.abs(np.cos(lattice.chain_momenta(6)[:, 0])) * 0.01, rtol=1e-2, atol=1e-12)
  # ops that do not begin with the translations: the first file alone
  result2 = dict(result, perms=perms[::-1].copy(), flips=flips[::-1].copy())
  assert [w.rsplit('/', 1)[1] for w in rs.write_files(str(tmp_path), hp, lattice.chain_bonds(6), labels[::-1], result2)] \
      == ['symmetries.txt']
  assert rs.momentum_weights_of(dict(result, flips=np.ones(14, np.uint8)), 6, 1) is None

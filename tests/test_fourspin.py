"""CPU: the four-spin (J-Q) terms -- the fp64 oracle tests/fourspin_oracle.py against dense exact diagonalisation of
H_J + H_Q, the term generators of lattice.py, the Q.txt files, operators.JQHamiltonian, cli_common.heisenberg_system, and
the host side of vmc_set_four_spin_terms (validation, pair table, pass planner) under AddressSanitizer +
UndefinedBehaviourSanitizer in a program of its own (csrc/hostcheck_fourspin.cpp)."""
import functools
import os
import re
import subprocess
import types

import numpy as np
import pytest

from cgs_vmc_amd import cli_common
from cgs_vmc_amd import lattice
from cgs_vmc_amd import operators
from tests import exact_states
from tests import fourspin_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORUS_BONDS = sorted({(min(i, j), max(i, j)) for i, j in lattice.torus_bonds(4, 4)})
SYSTEMS = {
    'chain8': (8, lattice.chain_bonds(8), lattice.jq_chain_terms(8)),
    'chain12': (12, lattice.chain_bonds(12), lattice.jq_chain_terms(12)),
    'torus4': (16, TORUS_BONDS, lattice.jq_torus_terms(4, 4)),
}
FRAMES = {'physical': (1.0, 1), 'rotated': (-1.0, -1)}      # (j_x, the exchange sign)


@functools.lru_cache(maxsize=None)
def _lowest(name, frame, q, k=1):
  n, bonds, terms = SYSTEMS[name]
  jx, sigma = FRAMES[frame]
  return fo.jq_lowest(n, bonds, jx, 1.0, terms, q, sigma, k=k)


@pytest.mark.parametrize('q', [0.0, 1.0, 2.5])
@pytest.mark.parametrize('frame', sorted(FRAMES))
@pytest.mark.parametrize('name', sorted(SYSTEMS))
def test_local_values_of_the_ground_state_are_its_energy(name, frame, q):
  """H v = E0 v, so the oracle's local energy of v is E0 on every configuration of the sector.  With the residual
  rho = ||H v - E0 v||_2 of the eigensolver's state, |E_loc(x) - E0| = |(H v - E0 v)(x)| / |v(x)| <= rho max |1 / v|: the
  tolerance, and nothing on top."""
  n, bonds, terms = SYSTEMS[name]
  jx, sigma = FRAMES[frame]
  w, v, basis, hmat = _lowest(name, frame, q)
  e0, vec = w[0], v[:, 0]
  assert (vec != 0).all()
  rho = np.linalg.norm(hmat @ vec - e0 * vec)
  inv = np.abs(1.0 / vec).max()
  tol = rho * inv
  psi = fo.Lookup(basis).psi(vec)
  eloc = fo.local_energy(psi, basis, bonds, jx, 1.0, terms, q, sigma)
  err = np.abs(eloc - e0).max()
  print('%s %s q = %g: E0 = %.9f, max |E_loc - E0| = %.3g, tolerance %.3g (residual %.3g, max |1 / v| %.3g)'
        % (name, frame, q, e0, err, tol, rho, inv))
  assert err <= tol
  if frame == 'rotated':                      # the rotated frame's ground state is strictly of one sign
    assert (vec > 0).all() or (vec < 0).all()
  if q == 0.0:                                # no terms: the Heisenberg ground state of tests/exact_states.py
    ref = exact_states.ed_ground_state(n, bonds, jx, 1.0)[0]
    assert abs(e0 - ref) <= 1e-10 * max(1.0, abs(ref))
    assert np.abs(fo.term_sums(psi, basis, terms, q, sigma)).max() == 0.0


@pytest.mark.parametrize('name', ['chain8', 'chain12'])
def test_both_frames_have_the_same_spectrum(name):
  a = _lowest(name, 'physical', 1.0, 2)[0]
  b = _lowest(name, 'rotated', 1.0, 2)[0]
  print('%s q = 1: E0 = %.6f, E1 = %.6f' % (name, a[0], a[1]))
  assert np.abs(a - b).max() <= 1e-10
  assert a[0] < a[1] - 0.1


def test_a_term_is_minus_q_times_the_product_of_two_singlet_projectors():
  """On four sites with one term: the matrix of the oracle's builder against the Kronecker products of spin-1/2 matrices
  restricted to Sz = 0, in both frames (the rotated frame flips the sign of S+ S- + h.c. on the two projector bonds)."""
  sx = np.array([[0, 0.5], [0.5, 0]]); sy = np.array([[0, -0.5j], [0.5j, 0]]); sz = np.diag([0.5, -0.5])

  def site(op, at):
    out = np.eye(1)
    for s in range(4):
      out = np.kron(out, op if s == at else np.eye(2))
    return out

  def projector(i, j, sigma):
    return 0.25 * np.eye(16) - (sigma * (site(sx, i) @ site(sx, j) + site(sy, i) @ site(sy, j)) + site(sz, i) @ site(sz, j))
  basis = fo.sz0_basis(4)
  # state index of a configuration: site 0 is the leftmost Kronecker factor, up (+1) is the first basis vector
  index = [int(''.join('0' if s > 0 else '1' for s in row), 2) for row in basis]
  for sigma in (1, -1):
    for term in ((0, 1, 2, 3), (2, 0, 3, 1)):
      dense = (-1.7 * projector(term[0], term[1], sigma) @ projector(term[2], term[3], sigma)).real
      mine = fo.jq_matrix(basis, [], [], [], [term], 1.7, sigma).toarray()
      np.testing.assert_allclose(mine, dense[np.ix_(index, index)], atol=1e-15)


def test_oracle_on_a_random_signed_vector_is_h_psi_over_psi():
  """Not an eigenstate, both signs, zero entries: the oracle's local energies times psi are H psi, 0 where psi vanishes."""
  n, bonds, terms = SYSTEMS['chain8']
  rng = np.random.default_rng(3)
  basis = fo.sz0_basis(n)
  vec = rng.standard_normal(len(basis))
  vec[::5] = 0.0
  q = rng.uniform(0.5, 2.0, len(terms)).astype(np.float32)
  for sigma in (1, -1):
    hmat = fo.jq_matrix(basis, bonds, 0.7 * sigma, 1.0, terms, q, sigma)
    eloc = fo.local_energy(fo.Lookup(basis).psi(vec), basis, bonds, 0.7 * sigma, 1.0, terms, q, sigma)
    np.testing.assert_allclose(eloc * vec, np.where(vec != 0, hmat @ vec, 0.0), atol=1e-12)
    assert (eloc[vec == 0] == 0).all()


def test_fold_emulation_agrees_with_the_plain_sum():
  n, bonds, terms = SYSTEMS['chain12']
  rng = np.random.default_rng(4)
  basis = fo.sz0_basis(n)
  vec = rng.uniform(0.5, 1.5, len(basis))
  cfg = basis[rng.permutation(len(basis))[:6]]
  parts = fo.term_parts(fo.Lookup(basis).psi(vec), cfg, terms, 1.25, -1)
  tp = parts['term_pairs']
  for c in range(len(cfg)):
    s = fo.fold_chain(parts['active'][:, c], parts['w'], parts['r1'][tp[:, 0], c], parts['r1'][tp[:, 1], c], parts['r2'][:, c], -1)
    assert abs(s - parts['value'][:, c].sum()) <= 1e-14 * np.abs(parts['products'][:, :, c]).sum()
  assert fo.fma(2.0 ** 53, 1.0 + 2.0 ** -52, -2.0 ** 53) == 2.0      # one rounding: the product alone would round to 2^53
  assert fo.butterfly(np.arange(64.0)) == 2016.0


# ---- the generators

def _translate_chain(terms, n, d):
  return (np.asarray(terms) + d) % n


def _translate_torus(terms, sx, sy, dx, dy):
  t = np.asarray(terms)
  return (t % sx + dx) % sx + sx * ((t // sx + dy) % sy)


def _canonical(terms):
  """A term as the set of its two unordered pairs: what the operator depends on."""
  return sorted(tuple(sorted((tuple(sorted((int(t[0]), int(t[1])))), tuple(sorted((int(t[2]), int(t[3]))))))) for t in terms)


@pytest.mark.parametrize('n', [4, 5, 8, 12, 66])
def test_chain_terms(n):
  terms = lattice.jq_chain_terms(n)
  assert terms.shape == (n, 4) and terms.dtype == np.int32
  assert all(len(set(t.tolist())) == 4 for t in terms) and terms.min() == 0 and terms.max() == n - 1
  bonds = {tuple(sorted(b)) for b in lattice.chain_bonds(n)}
  for t in terms:
    assert tuple(sorted((int(t[0]), int(t[1])))) in bonds and tuple(sorted((int(t[2]), int(t[3])))) in bonds
  for d in (1, 3):
    assert _canonical(_translate_chain(terms, n, d)) == _canonical(terms)
  assert len(set(map(tuple, terms.tolist()))) == n


@pytest.mark.parametrize('sx,sy', [(3, 3), (4, 4), (3, 5), (10, 10)])
def test_torus_terms(sx, sy):
  terms = lattice.jq_torus_terms(sx, sy)
  n = sx * sy
  assert terms.shape == (2 * n, 4) and terms.dtype == np.int32
  assert all(len(set(t.tolist())) == 4 for t in terms)
  coords = lattice.torus_coords(sx, sy)
  bonds = {tuple(sorted(b)) for b in lattice.torus_bonds(sx, sy)}
  horizontal = vertical = 0
  for t in terms:
    a, b = (int(t[0]), int(t[1])), (int(t[2]), int(t[3]))
    assert tuple(sorted(a)) in bonds and tuple(sorted(b)) in bonds
    # one plaquette: the four sites are {x, x + 1} x {y, y + 1} (periodically) of the first site
    x0, y0 = coords[t[0]]
    want = {(int((x0 + dx) % sx), int((y0 + dy) % sy)) for dx in (0, 1) for dy in (0, 1)}
    assert {(int(coords[s][0]), int(coords[s][1])) for s in t} == want
    # the two bonds are parallel
    da = (coords[a[1]] - coords[a[0]]) % (sx, sy); db = (coords[b[1]] - coords[b[0]]) % (sx, sy)
    assert (da == db).all() and sorted(da.tolist()) == [0.0, 1.0]
    horizontal += int(da[0] == 1); vertical += int(da[1] == 1)
  assert horizontal == n and vertical == n
  assert len(_canonical(terms)) == len(set(_canonical(terms))) == 2 * n
  for dx, dy in ((1, 0), (0, 1), (2, 1)):
    assert _canonical(_translate_torus(terms, sx, sy, dx, dy)) == _canonical(terms)


def test_generators_refuse_small_lattices():
  with pytest.raises(ValueError, match='n_sites >= 4'):
    lattice.jq_chain_terms(3)
  for size in ((2, 4), (4, 2), (1, 1)):
    with pytest.raises(ValueError, match='both sizes >= 3'):
      lattice.jq_torus_terms(*size)


# ---- Q.txt

def test_q_file_round_trip(tmp_path):
  terms = lattice.jq_torus_terms(4, 4)
  q = np.random.default_rng(1).uniform(-2, 2, len(terms)).astype(np.float32)
  path = str(tmp_path / 'Q.txt')
  lattice.write_four_spin_terms(path, terms, q)
  got_terms, got_q = lattice.read_four_spin_terms(path)
  np.testing.assert_array_equal(got_terms, terms); np.testing.assert_array_equal(got_q, q)
  assert got_terms.dtype == np.int32 and got_q.dtype == np.float32
  lattice.write_four_spin_terms(path, terms)                       # four columns: the reader's default
  got_terms, got_q = lattice.read_four_spin_terms(path, default_q=0.75)
  np.testing.assert_array_equal(got_terms, terms); assert (got_q == np.float32(0.75)).all()
  lattice.write_four_spin_terms(path, terms[:3], 2.5)               # a scalar
  assert lattice.read_four_spin_terms(path)[1].tolist() == [2.5, 2.5, 2.5]
  with open(path, 'w') as f:
    f.write('# comment\n\n0, 1, 2, 3   # trailing\n4 5 6 7 -1.5\n')
  got_terms, got_q = lattice.read_four_spin_terms(path, default_q=2.0)
  assert got_terms.tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]] and got_q.tolist() == [2.0, -1.5]
  assert lattice.load_four_spin_terms(str(tmp_path)) is not None
  assert lattice.load_four_spin_terms(str(tmp_path / 'nowhere')) is None


@pytest.mark.parametrize('text,match', [
    ('0 1 2\n', 'a line is a four-spin term'),
    ('0 1 2 3 1.0 7\n', 'a line is a four-spin term'),
    ('0 1 2 x\n', 'a line is a four-spin term'),
    ('0 1 2 3 nan\n', 'a line is a four-spin term'),
    ('0 1 2 3 q\n', 'a line is a four-spin term'),
    ('0 1 1 3\n', 'four distinct sites'),
    ('0 1 2 -3\n', 'four distinct sites'),
    ('# nothing\n', 'no four-spin term'),
])
def test_q_file_errors(tmp_path, text, match):
  path = tmp_path / 'Q.txt'
  path.write_text(text)
  with pytest.raises(ValueError, match=match):
    lattice.read_four_spin_terms(str(path))


def test_writer_refuses_bad_terms(tmp_path):
  for bad in ([[0, 1, 2]], [[0, 1, 2, 2]], [], [[0.5, 1, 2, 3]]):
    with pytest.raises(ValueError):
      lattice.write_four_spin_terms(str(tmp_path / 'Q.txt'), bad)
  with pytest.raises(ValueError, match=r'in 0 \.\. 7'):
    lattice.check_four_spin_terms([[0, 1, 2, 8]], 8)


# ---- operators.JQHamiltonian

def test_jq_hamiltonian_fields_and_defaults():
  bonds, terms = lattice.chain_bonds(8), lattice.jq_chain_terms(8)
  h = operators.JQHamiltonian(bonds, -1.0, 1.0, terms, 1.5)
  assert isinstance(h, operators.HeisenbergHamiltonian)
  assert h._exchange_sign == -1 and h._q.dtype == np.float32 and h._q.tolist() == [1.5] * 8
  np.testing.assert_array_equal(h._four_spin_terms, terms)
  assert h._bonds_list == [tuple(b) for b in bonds] and (h._j_x == -1).all() and (h._j_z == 1).all()
  assert operators.JQHamiltonian(bonds, 0.5, 1.0, terms, np.arange(8.0))._exchange_sign == 1
  per_bond = np.where(np.arange(8) % 2 == 0, 1.0, -1.0)
  assert operators.JQHamiltonian(bonds, per_bond, 1.0, terms, 1.0, exchange_sign=-1)._exchange_sign == -1
  assert operators.JQHamiltonian(bonds, 0.0, 1.0, terms, 1.0, exchange_sign=1)._exchange_sign == 1


def test_jq_hamiltonian_errors():
  bonds, terms = lattice.chain_bonds(8), lattice.jq_chain_terms(8)
  per_bond = np.where(np.arange(8) % 2 == 0, 1.0, -1.0)
  with pytest.raises(ValueError, match='do not share one sign of j_x'):
    operators.JQHamiltonian(bonds, per_bond, 1.0, terms, 1.0)
  with pytest.raises(ValueError, match='do not share one sign of j_x'):
    operators.JQHamiltonian(bonds, 0.0, 1.0, terms, 1.0)
  for sign in (0, 2, -3, 0.5):
    with pytest.raises(ValueError, match=r'exchange_sign is \+1 or -1'):
      operators.JQHamiltonian(bonds, 1.0, 1.0, terms, 1.0, exchange_sign=sign)
  with pytest.raises(ValueError, match='one value per term'):
    operators.JQHamiltonian(bonds, 1.0, 1.0, terms, [1.0, 2.0])
  with pytest.raises(ValueError, match='one value per term'):
    operators.JQHamiltonian(bonds, 1.0, 1.0, terms, np.ones((8, 1)))
  with pytest.raises(ValueError, match='finite'):
    operators.JQHamiltonian(bonds, 1.0, 1.0, terms, [1.0] * 7 + [np.inf])
  with pytest.raises(ValueError, match='four distinct sites'):
    operators.JQHamiltonian(bonds, 1.0, 1.0, [[0, 1, 1, 2]], 1.0)
  with pytest.raises(ValueError, match='four-spin terms'):
    operators.JQHamiltonian(bonds, 1.0, 1.0, [[0, 1, 2]], 1.0)
  with pytest.raises(ValueError, match='four-spin terms'):
    operators.JQHamiltonian(bonds, 1.0, 1.0, [], 1.0)


class _Engine:
  """What ConfigsVariable._ensure_hamiltonian calls on an engine."""
  n_four_spin_terms = 0

  def __init__(self):
    self.calls = []

  def set_bonds(self, bonds, j_x, j_z):
    self.calls.append(('bonds', len(bonds)))

  def set_four_spin_terms(self, terms, q, exchange_sign, rows_per_pass=0):
    self.n_four_spin_terms = len(terms)
    self.calls.append(('terms', len(terms), int(exchange_sign)))


def test_installing_uploads_the_terms_and_a_plain_hamiltonian_clears_them():
  from cgs_vmc_amd import graph_builders
  bonds, terms = lattice.chain_bonds(8), lattice.jq_chain_terms(8)
  var = types.SimpleNamespace(_hamiltonian=None, _engine=_Engine())
  ensure = lambda h: graph_builders.ConfigsVariable._ensure_hamiltonian(var, h)
  plain, jq = operators.HeisenbergHamiltonian(bonds, -1.0, 1.0), operators.JQHamiltonian(bonds, -1.0, 1.0, terms, 1.0)
  ensure(plain)
  assert var._engine.calls == [('bonds', 8)]                         # no terms, none to clear: exactly as before
  ensure(jq); ensure(jq)
  assert var._engine.calls[1:] == [('bonds', 8), ('terms', 8, -1)]
  ensure(plain)
  assert var._engine.calls[3:] == [('bonds', 8), ('terms', 0, 1)] and var._engine.n_four_spin_terms == 0
  ensure(operators.HeisenbergHamiltonian(bonds, 1.0, 1.0))
  assert var._engine.calls[5:] == [('bonds', 8)]


# ---- cli_common.heisenberg_system

def _hparams(n):
  from cgs_vmc_amd import utils
  hp = utils.create_hparams()
  hp.set_hparam('num_sites', n)
  hp.set_hparam('wavefunction_type', 'fully_connected')
  return hp


def test_heisenberg_system_with_and_without_q_file(tmp_path):
  hp = _hparams(8)
  _, h = cli_common.heisenberg_system(hp, str(tmp_path), -1.0)
  assert type(h) is operators.HeisenbergHamiltonian and h._bonds_list == [tuple(b) for b in lattice.chain_bonds(8)]
  lattice.write_four_spin_terms(str(tmp_path / 'Q.txt'), lattice.jq_chain_terms(8))
  _, h = cli_common.heisenberg_system(hp, str(tmp_path), -1.0)
  assert type(h) is operators.JQHamiltonian and h._exchange_sign == -1 and h._q.tolist() == [1.0] * 8
  np.testing.assert_array_equal(h._four_spin_terms, lattice.jq_chain_terms(8))
  _, h = cli_common.heisenberg_system(hp, str(tmp_path), 1.0, four_spin_q=0.25)
  assert h._exchange_sign == 1 and h._q.tolist() == [0.25] * 8
  lattice.write_four_spin_terms(str(tmp_path / 'Q.txt'), lattice.jq_chain_terms(8), 3.0)      # a fifth column wins
  assert cli_common.heisenberg_system(hp, str(tmp_path), 1.0, four_spin_q=0.25)[1]._q.tolist() == [3.0] * 8


def test_the_flag_is_taken_where_it_is_consumed_and_the_tables_stay(monkeypatch):
  """--four_spin_q: parsed by the three drivers that hand it to heisenberg_system, beside their FLAG_TABLE (which keeps
  the reference's contract); no other driver's parser knows it."""
  import importlib
  seen = []
  real = cli_common.parser_from_table

  def spy(doc, table):
    seen.append([row[0] for row in table])
    raise SystemExit(0)
  for name in ('run_training', 'run_energy_evaluation', 'run_excited_state_training'):
    module = importlib.import_module('cgs_vmc_amd.' + name)
    assert 'four_spin_q' not in {row[0] for row in module.FLAG_TABLE}
    monkeypatch.setattr(cli_common, 'parser_from_table', spy)
    with pytest.raises(SystemExit):
      module.main([])
    monkeypatch.setattr(cli_common, 'parser_from_table', real)
    assert seen[-1] == [row[0] for row in module.FLAG_TABLE] + ['four_spin_q']
    parser = real('', module.FLAG_TABLE + cli_common.FOUR_SPIN_FLAGS)
    assert parser.parse_args([]).four_spin_q == 1.0 and parser.parse_args(['--four_spin_q', '2.5']).four_spin_q == 2.5
  for name in ('run_lanczos_evaluation', 'run_projected_energy_evaluation', 'run_dimer_evaluation', 'run_overlap_evaluation',
               'run_symmetrized_training', 'run_symmetrized_energy_evaluation'):
    module = importlib.import_module('cgs_vmc_amd.' + name)
    with pytest.raises(SystemExit):
      real('', module.FLAG_TABLE).parse_args(['--four_spin_q', '2.5'])


def test_drivers_that_would_leave_the_terms_out_refuse_a_q_file(tmp_path):
  """run_lanczos_evaluation and run_projected_energy_evaluation build the Hamiltonian they measure from the bonds, and a
  symmetrized ctx takes no terms: on a directory with Q.txt each refuses before anything is built, and runs as before
  without the file (here: gets as far as the missing hparams.pbtxt)."""
  from cgs_vmc_amd import run_lanczos_evaluation as rl, run_projected_energy_evaluation as rp, run_symmetrized_training as rst
  d = str(tmp_path)
  calls = (
      lambda: rl.evaluate(cli_common.parser_from_table('', rl.FLAG_TABLE).parse_args(['--checkpoint_dir', d])),
      lambda: rp.evaluate(cli_common.parser_from_table('', rp.FLAG_TABLE).parse_args(['--checkpoint_dir', d])),
  )
  for call in calls:
    with pytest.raises((OSError, IOError)):
      call()
  lattice.write_four_spin_terms(str(tmp_path / 'Q.txt'), lattice.jq_chain_terms(8))
  for call, match in zip(calls, ('run_lanczos_evaluation: .*holds Q.txt', 'run_projected_energy_evaluation: .*holds Q.txt')):
    with pytest.raises(NotImplementedError, match=match):
      call()
  with pytest.raises(NotImplementedError, match='the symmetrized drivers: .*holds Q.txt'):
    rst.symmetrized_system(_hparams(8), d, 1.0, 'k0', lattice.translations(8), None, np.ones(8))


def test_make_ed_vector_writes_the_jq_ground_state(tmp_path):
  import importlib.util
  spec = importlib.util.spec_from_file_location('make_ed_vector', os.path.join(ROOT, 'tools', 'make_ed_vector.py'))
  tool = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(tool)
  for lattice_name, size, name in (('chain', ['8'], 'chain8'), ('square', ['4', '4'], 'torus4')):
    d = str(tmp_path / name)
    e0 = tool.main([d, '--lattice', lattice_name, '--size'] + size + ['--jx', '-1', '--jq', '1.0'])
    assert abs(e0 - _lowest(name, 'rotated', 1.0)[0][0]) <= 1e-9
    terms, q = lattice.read_four_spin_terms(os.path.join(d, 'Q.txt'))
    np.testing.assert_array_equal(terms, SYSTEMS[name][2]); assert (q == 1).all()
    vec = np.loadtxt(os.path.join(d, 'ed_vector.txt'))
    assert (vec > 0).all()
    _, h = cli_common.heisenberg_system(_hparams(SYSTEMS[name][0]), d, -1.0)
    assert type(h) is operators.JQHamiltonian and sorted(h._bonds_list) == sorted(tuple(b) for b in SYSTEMS[name][1])
  d = str(tmp_path / 'plain')
  tool.main([d, '--lattice', 'chain', '--size', '8'])
  assert not os.path.exists(os.path.join(d, 'Q.txt'))


def test_chain8_energies_of_the_jq_model():
  w = _lowest('chain8', 'rotated', 1.0, 2)[0]
  assert abs(w[0] + 8.324079) < 1e-6 and abs(w[1] + 6.297321) < 1e-6
  assert abs(_lowest('chain12', 'rotated', 1.0)[0][0] + 12.160136) < 1e-6


# ---- the C ABI and the host side

def test_engine_and_library_declare_the_entries():
  from cgs_vmc_amd import _hip
  from cgs_vmc_amd.engine import VmcEngine
  assert 'vmc_set_four_spin_terms' in _hip.SIGNATURES and 'vmc_last_four_spin_rows' in _hip.SIGNATURES
  assert callable(VmcEngine.set_four_spin_terms) and callable(VmcEngine.last_four_spin_rows)
  header = open(os.path.join(ROOT, 'include', 'cgsvmc.h')).read()
  assert 'int vmc_set_four_spin_terms(vmc_ctx* ctx, int32_t n_terms' in header


def test_host_side_under_asan_and_ubsan():
  p = subprocess.run(['make', '-C', os.path.join(ROOT, 'cgs_vmc_amd', 'csrc'), 'hostcheck_fourspin'],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
  out = p.stdout.decode()
  assert p.returncode == 0, out[-4000:]
  assert '-fsanitize=address,undefined' in out
  m = re.search(r'hostcheck_fourspin ok: (\d+) cases, (\d+) assertions', out)
  assert m, out[-2000:]
  assert int(m.group(1)) >= 400 and int(m.group(2)) > 10 ** 5

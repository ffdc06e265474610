"""CPU side of the symmetrized ansatz (wavefunctions.SymmetrizedWavefunction, vmc_create_symmetrized): the two identities on
the fp64 oracle, the wavefunction class (variables, names, deep copy, engine spec, the refusals that need no engine), the
sector files of the drivers, the host planner check, and what must NOT have changed (WAVEFUNCTION_TYPES, the hparams)."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

from cgs_vmc_amd import _hip, graph_builders, lattice, session, utils, wavefunctions
from oracle import vmc_oracle as vo
from tests import prod_oracle as pro
from tests import symmetrized_oracle as so
from tests import symmetrized_shape_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(8, 1, 'q0'), (8, 1, 'q4'), (4, 4, 'q0,0'), (4, 4, 'q2,2')]      # k = 0, k = pi, (0, 0), (pi, pi)


@pytest.fixture(autouse=True)
def _fresh_graph():
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  yield
  session.reset_default_graph(); wavefunctions.reset_name_scope()


def _oracle(sx, sy, sector, seed=1):
  n = sx * sy
  bonds = vo.chain_bonds(n) if sy == 1 else vo.torus_bonds(sx, sy)
  labels, chi = lattice.sector_characters(sx, sy)
  theta = vo.init_params(n, 16, 2, np.random.default_rng(seed))       # the 2 x 16 relu / exp network
  return so.Symmetrized(pro.fc_factor(theta, 16, 2), lattice.translations(sx, sy), None, chi[labels.index(sector)]), bonds


@pytest.mark.parametrize('sx,sy,sector', CASES)
def test_the_fold_of_the_base_local_energies_is_the_direct_local_energy(sx, sy, sector):
  """E_loc^s(x) = sum_k c_k(x) E_loc^psi(g_k x) against the direct sum over connected configurations of psi_s, in fp64."""
  orc, bonds = _oracle(sx, sy, sector)
  cfg = vo.random_configurations(sx * sy, 512, np.random.RandomState(2))
  cfg = cfg[orc.cancellation(cfg) > 1e-9]                 # (a structural zero has no local energy)
  assert len(cfg) >= 500
  for jx, jz in ((1.0, 1.0), (-1.0, 1.0), (0.7, 1.3)):
    direct = orc.local_energy(cfg, bonds, jx, jz)
    fold = orc.local_energy_fold(cfg, bonds, jx, jz)
    # (scaled by the cancellation: the error of either side grows as 1 / r, the identity holds to rounding times that)
    rel = np.abs((direct - fold) * orc.cancellation(cfg)).max() / np.abs(direct).max()
    assert rel <= 1e-12, (sector, jx, jz, rel)
  w = orc.weights(cfg)
  np.testing.assert_allclose(w.sum(0), 1.0, rtol=0, atol=1e-9)


@pytest.mark.parametrize('sx,sy,sector', CASES)
def test_covariance_and_log_derivatives_of_the_oracle(sx, sy, sector):
  orc, _ = _oracle(sx, sy, sector)
  n = sx * sy
  cfg = vo.random_configurations(n, 32, np.random.RandomState(3))
  psi, a = orc.psi(cfg), orc.A(cfg)
  rows = orc.rows(cfg)
  for k in range(orc.n_ops):                              # psi_s(g_k x) = chi_k / chi_0 psi_s(x)
    np.testing.assert_allclose(orc.psi(rows[k]), orc.chi[k] / orc.chi[0] * psi, rtol=0, atol=1e-12 * a.max())
  # O^s against central differences of ln|psi_s| in a few parameters
  keep = orc.cancellation(cfg) > 0.05
  o = orc.log_grads(cfg[keep])
  base = orc.base
  for j in (0, 5, base.num_params - 1):
    h = 1e-6
    vals = []
    for s in (+1, -1):
      th = base.theta.copy(); th[j] += s * h
      vals.append(np.log(np.abs(so.Symmetrized(pro.fc_factor(th, 16, 2), orc.perms, None, orc.chi).psi(cfg[keep]))))
    np.testing.assert_allclose(o[:, j], (vals[0] - vals[1]) / (2 * h), rtol=1e-5, atol=1e-6)


def test_structural_zeros_of_the_flip_sectors():
  """A Neel row is a zero of (k = pi, flip-even) and (k = 0, flip-odd), whatever psi is: an op with character -1 maps it
  onto itself.  Under the translations alone (k = pi) it is none."""
  neel = np.array([[1, -1] * 4], np.float32)
  theta = vo.init_params(8, 16, 2, np.random.default_rng(4))
  fac = pro.fc_factor(theta, 16, 2)
  t = lattice.translations(8)
  labels, chi = lattice.sector_characters(8, 1, spin_flip=True)
  perms, flips = np.concatenate([t, t]), np.repeat([0, 1], 8)
  for sector, zero in (('q4+', True), ('q0-', True), ('q0+', False), ('q4-', False)):
    r = so.Symmetrized(fac, perms, flips, chi[labels.index(sector)]).cancellation(neel)[0]
    assert (r < 1e-14) == zero, (sector, r)
  labels, chi = lattice.sector_characters(8, 1)
  assert so.Symmetrized(fac, t, None, chi[labels.index('q4')]).cancellation(neel)[0] > 1e-6


def test_sector_levels_of_the_eight_site_chain():
  t = lattice.translations(8)
  labels, chi = lattice.sector_characters(8, 1)
  bonds = vo.chain_bonds(8)
  e_pi = so.sector_hamiltonian_levels(8, bonds, 1.0, 1.0, t, None, chi[labels.index('q4')])
  e_0 = so.sector_hamiltonian_levels(8, bonds, 1.0, 1.0, t, None, chi[labels.index('q0')])
  assert abs(e_pi[0] + 3.1284) < 1e-4 and abs(e_0[0] + 3.6511) < 1e-4
  total = sum(len(so.sector_hamiltonian_levels(8, bonds, 1.0, 1.0, t, None, c)) for c in chi)
  assert total == 70                                       # the sectors partition the Sz = 0 block


# ---- the inputs of tests/test_gpu_symmetrized_shapes.py, on the oracle alone

SHAPE_OP_SETS = sorted({(lat, sector) for _, lat, sector, _ in sc.AMPLITUDE_CASES} | {(lat, sector) for lat, sector, _ in sc.GRADIENT_CASES})


@pytest.mark.parametrize('lat,sector', SHAPE_OP_SETS)
def test_the_fold_identity_holds_on_every_shape_case(lat, sector):
  """Direct sum against fold with the 2 x 16 oracle factor on every op set of the shape cases -- N up to 258, the spin flip,
  a rectangle, the 128 ops of the space group, two couplings --, r-scaled as above: 1e-12 max(1, max|E|)."""
  L = sc.LATTICES[lat]
  perms, flips, chi = sc.ops(lat, sector)                  # (validated against the bonds and couplings there)
  assert len(perms) == {'chain10': 10, 'chain12': 24, 'chain20': 20, 'chain68': 68, 'chain258': 6, 'torus6x4': 24,
                        'torus4': 128, 'torus4-j1j2': 128}.get(lat, 140 if flips is not None else 70)
  orc = sc.fc_oracle(lat, sector, sc.fc_theta(L['n'], 1))
  cfg = sc.configs(L['n'], 5 if L['n'] > 64 else 8, 2, orc)
  r = orc.cancellation(cfg)
  for jx, jz in ((1.0, 1.0), (0.7, 1.3)):
    bx, bz = sc.couplings(lat, jx, jz)
    direct = orc.local_energy(cfg, L['bonds'], bx, bz)
    fold = orc.local_energy_fold(cfg, L['bonds'], bx, bz)
    assert (r * np.abs(direct - fold)).max() <= 1e-12 * max(1.0, np.abs(direct).max()), (lat, sector, jx, jz)
  if lat == 'torus4-j1j2':                                 # the two couplings are what makes the ops symmetries: swap two and they are not
    j = np.array(L['j']); j[0], j[40] = j[40], j[0]
    with pytest.raises(ValueError, match='no symmetry of the Hamiltonian'):
      lattice.check_hamiltonian_symmetry(L['bonds'], j, j, perms)


@pytest.mark.parametrize('name', ['trivial', 'sign', 'A2'])
def test_the_space_group_sectors_are_representations(name):
  """chi(g) chi(h) = chi(g h) / |G| on the 128 x 128 table of the 4 x 4 torus' space group, and on the oracle
  psi_s(g_k x) = chi_k / chi_0 psi_s(x) to 1e-12 A."""
  perms, flips, chi = sc.ops('torus4', 'sg-' + name)
  g = len(perms)
  assert g == 128 and flips is None and (np.abs(chi) == 1.0 / g).all() and chi[0] > 0
  assert (chi < 0).sum() == {'trivial': 0, 'sign': 64, 'A2': 64}[name]
  index = {p.tobytes(): k for k, p in enumerate(perms)}
  assert len(index) == g and index[np.arange(16, dtype=np.int32).tobytes()] == 0
  # rows: x -> x[perm_a] -> (x[perm_a])[perm_b] = x[perm_a[perm_b]]
  table = np.array([[index[perms[a][perms[b]].tobytes()] for b in range(g)] for a in range(g)])      # (a KeyError: not closed)
  assert (np.sort(table, axis=1) == np.arange(g)).all()
  assert (table != table.T).any()                          # the group does not commute
  np.testing.assert_array_equal(chi[:, None] * chi[None, :], chi[table] / g)
  orc = sc.fc_oracle('torus4', 'sg-' + name, sc.fc_theta(16, 1))
  cfg = sc.configs(16, 8, 3)
  psi, a = orc.psi(cfg), orc.A(cfg)
  rows = orc.rows(cfg)
  for k in range(g):
    np.testing.assert_allclose(orc.psi(rows[k]), chi[k] / chi[0] * psi, rtol=0, atol=1e-12 * a.max())


@pytest.mark.parametrize('lat,sector,b', sc.GRADIENT_CASES)
def test_the_gradient_seed_table_keeps_r_min(lat, sector, b):
  """Every (parameter seed, batch seed) of the GPU gradient tests: min_c r >= 0.01 on the unfiltered batch the seeds pick."""
  theta_seed, seed = sc.GRADIENT_SEEDS[(lat, sector, b)]
  n = sc.LATTICES[lat]['n']
  orc = sc.fc_oracle(lat, sector, sc.fc_theta(n, theta_seed))
  r = orc.cancellation(sc.configs(n, b, seed, orc))
  assert r.min() >= sc.R_MIN, (lat, sector, r)


def test_the_shape_cases_reach_what_they_are_named_for():
  """What the GPU tests assert before they run, where it needs no GPU: the sizes, the logit spreads of the fold cases,
  the rows of the zero-amplitude batches, the band share of the big injected step."""
  n = lambda lat: sc.LATTICES[lat]['n']
  assert n('chain10') % 4 == 2 and n('chain70') % 4 == 2 and n('chain68') % 4 == 0 and min(n('chain68'), n('chain70')) > 64
  assert (n('chain258') + 3) // 4 == 65 and n('chain258') % 4 == 2
  big = sc.BIG
  assert len(sc.ops(big['lat'], big['sector'])[0]) * big['b'] > sc.ROW_ITEMS_PER_CU * 256      # (at the MI355X's 256 CUs)
  assert sc.FOLD_THREADS < big['b'] < 2 * sc.FOLD_THREADS
  plan = open(os.path.join(ROOT, 'cgs_vmc_amd', 'csrc', 'plan.hpp')).read()
  common = open(os.path.join(ROOT, 'cgs_vmc_amd', 'csrc', 'measure_dev.hpp')).read()      # (where measure_rows_grid lives)
  assert re.search(r'#define\s+PLAN_SYMZ_THREADS\s+%d\b' % sc.FOLD_THREADS, plan)
  assert 'long long blocks = (items + 3) / 4;' in common and 'const long long cap = 16LL * (num_cus > 0 ? num_cus : 1);' in common
  # the fold cases: every row's orbit spreads past the range its factor is named for
  for lat, sector in sc.FOLD_CASES:
    for factor, spread in sc.FOLD_FACTORS.items():
      theta = sc.fold_theta(n(lat), factor)
      orc = sc.fc_oracle(lat, sector, theta)
      l = sc.orbit_logits(theta, orc, sc.configs(n(lat), 5, sc.FOLD_SEED))
      assert (l.max(0) - l.min(0) > 1.05 * spread).all(), (lat, factor, l.max(0) - l.min(0))
  # zero characters: rows on which an odd translation's logit lies past fp64's exp range above every even one's
  bare = sc.fold_theta(8, sc.ZERO_CHI_FACTOR)
  l = sc.orbit_logits(bare, sc.fc_oracle('chain8', 'q0', bare), sc.configs(8, 13, sc.ZERO_CHI_SEED + 1))
  assert (l[1::2].max(0) - l[0::2].max(0) > 1.05 * 745.0).sum() >= 2
  # the zero-amplitude batches: a row with some but not all ops on a zero entry, every row with psi_s != 0
  vec, top, bot = sc.zero_vector()
  assert 0.25 * len(vec) < (vec == 0).sum() < 0.5 * len(vec)
  for sector in sc.ZERO_AMP['sectors']:
    perms, flips, chi = sc.ops('chain8', sector)
    orc = so.Symmetrized(pro.edvec_factor(vec, top, bot), perms, flips, chi)
    cfg, partial = sc.zero_amp_batch(orc)
    assert len(cfg) == sc.ZERO_AMP['b'] and partial.any() and (orc.cancellation(cfg) > 1e-3).all()
    assert (orc.terms(sc.DOMAIN_WALL[None]) == 0).all()
  # the big injected step: the oracle alone keeps the band share
  orc = sc.fc_oracle(big['lat'], big['sector'], sc.fc_theta(n(big['lat']), 0))
  cfg = sc.configs(n(big['lat']), big['b'], big['seed'], orc)
  i_up, i_dn, u = sc.big_step(cfg)
  _, acc, ratio = pro.mc_step(orc, cfg, i_up, i_dn, u)
  band = ~(np.abs(ratio ** 2 - u.astype(np.float64)) > 2e-4)
  assert band.sum() <= sc.BAND_SHARE * big['b'] and 0.2 * big['b'] < acc.sum() < 0.9 * big['b']
  # exact zeros where q2 of the 8-site chain should have them, and otherwise lattice.sector_characters' row
  labels, table = lattice.sector_characters(8, 1)
  assert (table[labels.index('q2')] != 0).all()
  np.testing.assert_allclose(sc.CHI_Q2_EXACT, table[labels.index('q2')], rtol=0, atol=1e-16)


def _base(n=8, **kw):
  hp = utils.create_hparams(wavefunction_type='fully_connected', num_sites=n, num_fc_layers=2, fc_layer_size=16, **kw)
  return wavefunctions.build_wavefunction(hp)


def test_the_variables_are_the_bases_and_the_deep_copy_works():
  base = _base()
  labels, chi = lattice.sector_characters(8, 1)
  wf = wavefunctions.SymmetrizedWavefunction(base, lattice.translations(8), None, chi[labels.index('q4')])
  assert wf._sub_wavefunctions == [base] and wf.n_ops == 8
  assert wf._unique_name == 'symmetrized_' + base._unique_name
  assert wf._exp_norm_shift is None and wf.update_norm(None) is None and wf.normalize_batch(None) is None
  base._n_sites = 8
  base.initialize(0)
  names = [v.name for v in wf.get_trainable_variables()]
  assert names == [v.name for v in base.get_trainable_variables()]
  assert names[0] == 'fully_connected_network/linear/w' and all(n.split('/')[0] == base._unique_name for n in names)
  assert wf._has_values and wf._theta is None
  twin = copy.deepcopy(wf)
  assert isinstance(twin, wavefunctions.SymmetrizedWavefunction) and twin._unique_name == 'dc_' + wf._unique_name
  assert twin._base is not base and twin._base._unique_name == 'dc_' + base._unique_name
  np.testing.assert_array_equal(twin._perms, wf._perms); np.testing.assert_array_equal(twin._chi, wf._chi)
  assert twin._flips is None and twin.ops_digest() == wf.ops_digest()
  twin._base._n_sites = 8
  twin._base._set_theta(np.zeros(twin._base.num_params, np.float32))
  session.Session().run(wavefunctions.module_transfer_ops(wf, twin))
  for s, d in zip(wf.get_trainable_variables(), twin.get_trainable_variables()):
    np.testing.assert_array_equal(d.eval(), s.eval())
  # the engine spec: the ansatz, the base's frozen spec, the ops and their digest
  spec = wf._engine_spec()
  assert spec['ansatz'] == 'symmetrized' and spec['base'] == tuple(sorted(base._engine_spec().items()))
  assert spec['ops_digest'] == wf.ops_digest() and len(spec['ops_digest']) == 64
  assert np.frombuffer(spec['ops'][0], np.int32).reshape(8, 8).tolist() == lattice.translations(8).tolist()
  other = wavefunctions.SymmetrizedWavefunction(_base(), lattice.translations(8), None, chi[labels.index('q0')])
  assert other.ops_digest() != wf.ops_digest() and other._engine_spec() != spec


def test_refusals_that_need_no_engine():
  t = lattice.translations(8)
  with pytest.raises(NotImplementedError, match='symmetrized'):
    wavefunctions.SymmetrizedWavefunction(1.0, t)
  conv = wavefunctions.build_wavefunction(utils.create_hparams(wavefunction_type='conv_1d', num_sites=8))
  with pytest.raises(NotImplementedError, match='Conv1DNetwork'):
    wavefunctions.SymmetrizedWavefunction(conv, t)
  prod = _base() * _base()
  with pytest.raises(NotImplementedError, match='product'):
    wavefunctions.SymmetrizedWavefunction(prod, t)
  inner = wavefunctions.SymmetrizedWavefunction(_base(), t)
  with pytest.raises(NotImplementedError, match='symmetrized'):
    wavefunctions.SymmetrizedWavefunction(inner, t)
  with pytest.raises(NotImplementedError, match='SymmetrizedWavefunction'):
    wavefunctions.ProductOfWavefunctions(inner, _base())
  bad = t.copy(); bad[2, 1] = bad[2, 0]
  with pytest.raises(ValueError, match='op 2'):
    wavefunctions.SymmetrizedWavefunction(_base(), bad)
  with pytest.raises(ValueError, match='flip'):
    wavefunctions.SymmetrizedWavefunction(_base(), t, [0, 2, 0, 0, 0, 0, 0, 0])
  with pytest.raises(ValueError, match='character'):
    wavefunctions.SymmetrizedWavefunction(_base(), t, None, np.ones(7))
  with pytest.raises(ValueError, match='not finite'):
    wavefunctions.SymmetrizedWavefunction(_base(), t, None, np.r_[np.nan, np.ones(7)])
  with pytest.raises(ValueError, match='zero'):
    wavefunctions.SymmetrizedWavefunction(_base(), t, None, np.zeros(8))
  with pytest.raises(ValueError, match='Hparams'):
    wavefunctions.SymmetrizedWavefunction.from_hparams(utils.create_hparams())
  # at bind time, before an engine is asked for: a non-exp dense base, a lattice of another size
  configs = graph_builders.get_configs({}, 4, 8)
  tanh = wavefunctions.SymmetrizedWavefunction(_base(output_activation='tanh'), t)
  with pytest.raises(NotImplementedError, match='exp output activation'):
    tanh(configs)
  with pytest.raises(ValueError, match='8 sites'):
    wavefunctions.SymmetrizedWavefunction(_base(), t)(graph_builders.get_configs({}, 4, 16))
  assert configs._engine is None
  with pytest.raises(ValueError, match='CONFIGS variable first'):
    wavefunctions.SymmetrizedWavefunction(_base(), t)(np.ones((2, 8), np.float32))


def test_sector_files_round_trip(tmp_path):
  from cgs_vmc_amd import run_symmetrized_energy_evaluation as rse, run_symmetrized_training as rst
  t = lattice.translations(4, 4)
  labels, chi = lattice.sector_characters(4, 4, spin_flip=True)
  perms, flips = np.concatenate([t, t]), np.repeat([0, 1], 16).astype(np.uint8)
  d = str(tmp_path)
  rst.write_sector(d, 'q2,2-', perms, flips, chi[labels.index('q2,2-')])
  assert sorted(os.listdir(d)) == ['sector_characters.txt', 'sector_ops.txt']
  label, p, f, c = rst.read_sector(d, 16)
  assert label == 'q2,2-'
  np.testing.assert_array_equal(p, perms); np.testing.assert_array_equal(f, flips)
  np.testing.assert_array_equal(c, chi[labels.index('q2,2-')])          # 17 significant digits: the same float64
  with pytest.raises(ValueError):
    rst.read_sector(d, 8)
  # the drivers' flags: run_training's plus the sector; the default lattice and the named row
  flags = rst.cli_common.parser_from_table('', rst.FLAG_TABLE).parse_args(
      ['--checkpoint_dir', d, '--num_sites', '8', '--sector', 'q4', '--wavefunction_type', 'fully_connected'])
  assert flags.optimizer == 'EnergyGradient' and not flags.spin_flip
  hp = rst.run_training.hparams_from_flags(flags)
  label, p, f, c = rst.choose_sector(flags, hp, lattice.chain_bonds(8))
  assert label == 'q4' and len(p) == 8 and not f.any()
  np.testing.assert_allclose(c, np.cos(np.pi * np.arange(8)) / 8, atol=1e-15)
  flags.sector = 'q9'
  with pytest.raises(ValueError, match='q9'):
    rst.choose_sector(flags, hp, lattice.chain_bonds(8))
  flags.optimizer = 'ITSWO'
  with pytest.raises(NotImplementedError, match='EnergyGradient'):
    rst.train(flags, hp)
  assert {row[0] for row in rse.FLAG_TABLE} == {'heisenberg_jx', 'checkpoint_dir', 'sector_dir', 'hparams'}
  # an op that is no symmetry of the bonds is refused before any engine exists
  with pytest.raises(ValueError, match='no symmetry of the Hamiltonian'):
    lattice.write_bonds(d, lattice.chain_bonds(8)[:-1])
    rst.symmetrized_system(hp, d, 1.0, 'q4', p, f, c)


def test_what_must_not_change():
  assert 'symmetrized' not in wavefunctions.WAVEFUNCTION_TYPES and 'symmetrized' not in _hip.ANSATZ_IDS
  keys = set(utils.create_hparams().values())
  assert not any(word in k for k in keys for word in ('sector', 'symmetr', 'character'))
  with pytest.raises(NotImplementedError):
    _base() + _base()
  assert _hip.ANSATZ_SYMMETRIZED == 13 and _hip.ANSATZ_PRODUCT == 11 and 12 not in _hip.ANSATZ_IDS.values()
  assert 8 not in _hip.ANSATZ_IDS.values() and _hip.PATH_SYMMETRIZED == 11
  header = open(os.path.join(ROOT, 'include', 'cgsvmc.h')).read()
  assert 'VMC_ANSATZ_SYMMETRIZED = 13' in header and 'int vmc_create_symmetrized(' in header
  assert 'vmc_create_symmetrized' in _hip.SIGNATURES and len(_hip.SIGNATURES['vmc_create_symmetrized'][1]) == 7
  plan = open(os.path.join(ROOT, 'cgs_vmc_amd', 'csrc', 'plan.hpp')).read()
  assert 'PATH_SYMMETRIZED = 11' in plan and 'PLAN_SYMZ_ZERO 0x1p-40' in plan


def test_host_planner_check_under_sanitizers():
  p = subprocess.run(['make', '-C', os.path.join(ROOT, 'cgs_vmc_amd', 'csrc'), 'hostcheck_symz'],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
  out = p.stdout.decode()
  assert p.returncode == 0, out[-4000:]
  assert '-fsanitize=address,undefined' in out
  assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
  m = re.search(r'hostcheck_symz ok: (\d+) cases, (\d+) assertions', out)
  assert m, out[-2000:]
  assert int(m.group(1)) >= 300 and int(m.group(2)) >= 500

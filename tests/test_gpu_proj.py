"""GPU: symmetry-projected energies (vmc_projected_energy: csrc/vmc_api_measure.hip + proj.hip; ProjectedEnergyEvaluator;
run_projected_energy_evaluation) against the fp64 oracle tests/proj_oracle.py.

Bounds (tests/proj_oracle.py: bounds).  w_sum[s] is linear in the per-op sums of tests/test_gpu_symm.py, so its bound is
sum_k |chi[s][k]| times that test's per-op bound; we_sum[s] carries the reference's |E_loc| through the same figure, adds
sum_c |w_ref(c)| dE(c) and the fp64 fold term, where dE is the tolerance the family's OWN local-energy parity test applies
(`_eloc_reference` below, each next to the file it is taken from).  No case is left out.

Measured on an MI355X, worst error / bound over the sectors (w_sum, we_sum): fully_connected 2.2e-4, 1.4e-4; rbm 5.1e-4,
4.4e-4; conv_2d 4.2e-3, 3.4e-3; gnn 3.0e-3, 1.9e-3; pbdg 1.3e-4, 2.8e-4; fully_connected_nnb 7.0e-4, 1.3e-3; ed_vector
0.22, 7.2e-3 (its amplitude bound is one fp32 spacing of the logs); 72 sites, 144 ops, 74 sectors, 200 chains: 1.8e-4,
3.1e-5.  The exact 4 x 4 ground state: |we_sum[s0] - E0 n_alive| = 1.6e-6 against 7.2e-4.  The sampled mixture (1,024
chains, 16 samples, 2 sweeps apart): E(0,+) = -3.65043 +- 0.0016 (cap 0.006), E(4,-) = -3.1345 +- 0.0142 (cap 0.06),
weights 0.9020 +- 0.0019 and 0.0980 +- 0.0019, unprojected -3.59986 +- 0.0010."""
import functools

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from cgs_vmc_amd import lattice
from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo
from tests import nnb_oracle as no
from tests import pbdg_oracle as po
from tests import proj_oracle as pj
from tests import test_gpu_renyi as tr

pytestmark = pytest.mark.gpu
N, H, B = tr.N, tr.H, tr.B                  # 4 x 4 torus, H = 32, 40 chains: no multiple of the 8- or 16-chain tiles
FAMILIES = tr.FAMILIES
BONDS = tr.BONDS
U24 = 2.0 ** -24


def _ops7():
  """identity, T(1,0), T(0,1), rot90, mirror_x, the flip alone, T(1,1) + flip: all symmetries of the 4 x 4 torus."""
  t = lattice.translations(4, 4)
  labels, group = lattice.point_group(4, 4)
  perms = np.stack([t[0], t[1], t[4], group[labels.index('rot90')], group[labels.index('mirror_x')], t[0], t[5]])
  return perms, np.array([0, 0, 0, 0, 0, 1, 1], np.uint8)


PERMS, FLIPS = _ops7()
# five rows of fixed random characters and the trivial sector
CHI = np.concatenate([np.random.default_rng(5).standard_normal((5, len(PERMS))), np.full((1, len(PERMS)), 1.0 / len(PERMS))])


def _eloc_reference(ansatz, theta, psi, cfg, bonds=BONDS, n_layers=2, h=H):
  """(E_loc fp64 [B], dE [B]): the oracle's local energies at j_x = j_z = 1 and the tolerance the family's own
  local-energy parity test applies to them; 0 / 0 for a chain whose own amplitude vanishes (never read)."""
  cfg = np.asarray(cfg, np.float32)
  if ansatz == 'pbdg':
    ref = po.local_energy(theta, cfg, bonds, 1.0, 1.0)
    # tests/test_gpu_pbdg.py: assert_allclose(eloc, ref, rtol=2e-3, atol=2e-3 mean |ref|)
    return ref, 2e-3 * np.abs(ref) + 2e-3 * np.abs(ref).mean()
  if ansatz == 'fully_connected_nnb':
    ref = no.local_energy(theta, cfg, bonds, 1.0, 1.0, n_layers, h)
    # tests/test_gpu_nnb.py (test_nnb_local_energy...): assert_allclose(eloc, ref, rtol=2e-3, atol=2e-3 mean |ref|)
    return ref, 2e-3 * np.abs(ref) + 2e-3 * np.abs(ref).mean()
  if ansatz == 'ed_vector':
    top, bot, _ = eo.lin_tables(cfg.shape[1])
    alive = eo.amplitude(theta, cfg, top, bot) != 0
    ref, tol = np.zeros(len(cfg)), np.zeros(len(cfg))
    diag, terms = eo.local_energy_terms(theta, cfg[alive], top, bot, bonds, 1.0, 1.0)
    # tests/test_gpu_edvec.py (_eloc_bound): (n_b + 3) 2^-24 (|diag| + sum |terms|)
    ref[alive] = diag + terms.sum(1)
    tol[alive] = ((terms != 0).sum(1) + 3) * U24 * (np.abs(diag) + np.abs(terms).sum(1))
    return ref, tol
  # tests/test_gpu_engine.py, test_gpu_rbm.py, test_gpu_conv.py, test_gpu_gnn.py: _close(eloc, ref, 2e-4) =
  # |d| <= 2e-4 max(1, |ref|)
  ref = vo.local_value(psi, cfg, bonds, 1.0, 1.0, dtype=np.float64)
  return ref, 2e-4 * np.maximum(1.0, np.abs(ref))


def _check(tag, got, psi, eps, eloc, d_eloc, cfg, perms, flips, chi):
  """Every output of one call against the oracle within the bounds; -> (ref, (w, we, e) bounds)."""
  ref = pj.sums(psi, eloc, cfg, perms, flips, chi)
  wb, web, eb = pj.bounds(psi, eps, eloc, d_eloc, cfg, perms, flips, chi)
  assert got['n_alive'] == ref['n_alive'], (tag, got['n_alive'], ref['n_alive'])
  assert np.isfinite(got['w_sum']).all() and np.isfinite(got['we_sum']).all() and np.isfinite(got['e_sum'])
  ew, ewe, ee = np.abs(got['w_sum'] - ref['w_sum']), np.abs(got['we_sum'] - ref['we_sum']), abs(got['e_sum'] - ref['e_sum'])
  assert (wb > 0).all() and (web > 0).all() and eb > 0
  print('%s: worst error / bound: w_sum %.3g, we_sum %.3g, e_sum %.3g (%d sectors, %d alive)'
        % (tag, (ew / wb).max(), (ewe / web).max(), ee / eb, len(wb), ref['n_alive']))
  assert (ew <= wb).all(), (tag, 'w_sum', int(np.argmax(ew / wb)), ew.max())
  assert (ewe <= web).all(), (tag, 'we_sum', int(np.argmax(ewe / web)), ewe.max())
  assert ee <= eb, (tag, 'e_sum', ee, eb)
  return ref, (wb, web, eb)


@pytest.mark.parametrize('ansatz', FAMILIES)
def test_sums_match_the_fp64_oracle(ansatz):
  theta, psi, eps = tr._family(ansatz)
  cfg = tr._cfg(2)
  eng = tr._engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(BONDS, 1.0, 1.0)
  got = eng.projected_energy(PERMS, FLIPS, CHI)
  eloc, d_eloc = _eloc_reference(ansatz, theta, psi, cfg)
  ref, _ = _check(ansatz, got, psi, eps, eloc, d_eloc, cfg, PERMS, FLIPS, CHI)
  assert (ref['n_alive'] < B) == (ansatz == 'ed_vector')      # the zeroed entries are met, and only there
  # the local energies the call leaves are vmc_local_energy's; flips = None is no flips; the supervisor's set measures too
  alive = psi(cfg) != 0
  left = eng.local_energy()[0][alive].astype(np.float64)
  assert abs(left.sum() - got['e_sum']) <= B * 2.0 ** -53 * np.abs(left).sum()     # (the same values in another order)
  five = eng.projected_energy(PERMS[:5], None, CHI[:, :5])
  again = eng.projected_energy(PERMS[:5], np.zeros(5, np.uint8), CHI[:, :5])
  for key in got:
    np.testing.assert_array_equal(five[key], again[key])
  eng.set_params(theta, _hip.VMC_OMEGA)
  omega = eng.projected_energy(PERMS, FLIPS, CHI, which=_hip.VMC_OMEGA)
  for key in got:
    np.testing.assert_array_equal(omega[key], got[key])
  eng.close()


def _same(a, b, msg=''):
  assert set(a) == set(b)
  for key in a:
    np.testing.assert_array_equal(a[key], b[key], err_msg='%s %s' % (msg, key))


def test_passes_repeats_sector_lists_and_tiles_are_bit_identical():
  theta, _, _ = tr._family('fully_connected')
  eng = tr._engine()
  eng.set_params(theta); eng.set_configs(tr._cfg(7)); eng.set_bonds(BONDS, 1.0, 1.0)
  base = eng.projected_energy(PERMS, FLIPS, CHI)
  for per in (1, 3, 0):
    for _ in range(2):
      _same(eng.projected_energy(PERMS, FLIPS, CHI, ops_per_pass=per), base, 'ops_per_pass=%d' % per)
  # a sector's sums do not depend on which other sectors are in the call, or where
  pick = np.array([4, 1, 5])
  sub = eng.projected_energy(PERMS, FLIPS, CHI[pick], ops_per_pass=3)
  np.testing.assert_array_equal(sub['w_sum'], base['w_sum'][pick]); np.testing.assert_array_equal(sub['we_sum'], base['we_sum'][pick])
  assert sub['e_sum'] == base['e_sum'] and sub['n_alive'] == base['n_alive']
  # 37 sectors: three sector tiles of 16, the last one partly filled, against the same sectors one call each
  many = np.random.default_rng(6).standard_normal((37, len(PERMS)))
  tiled = eng.projected_energy(PERMS, FLIPS, many, ops_per_pass=2)
  for s in range(len(many)):
    one = eng.projected_energy(PERMS, FLIPS, many[s])
    assert one['w_sum'][0] == tiled['w_sum'][s] and one['we_sum'][0] == tiled['we_sum'][s], s
  eng.close()


@functools.lru_cache(maxsize=None)
def _torus_ground_state():
  return eo.vector_from_ed(N, BONDS, 1.0, 1.0)


def _translation_sectors(size_x, size_y):
  t = lattice.translations(size_x, size_y)
  labels, chi = lattice.sector_characters(size_x, size_y, True)
  return labels, np.concatenate([t, t]), np.repeat([0, 1], len(t)).astype(np.uint8), chi


def test_an_exact_eigenstate_lives_in_one_sector_with_its_energy():
  """The 4 x 4 ground state (j_x = +1) in ed_vector: momentum 0 and even under the flip, so w_s(c) = 1 in that sector and 0
  in every other on every chain, whatever the chains, and E_loc = E0."""
  e0, vec64, top, bot = _torus_ground_state()
  vec = vec64.astype(np.float32)
  labels, perms, flips, chi = _translation_sectors(4, 4)
  s0 = labels.index('q0,0+')
  cfg = tr._cfg(4)
  psi = lambda c: eo.amplitude(vec.astype(np.float64), c, top, bot)
  eps = tr._edvec_eps(vec, top, bot)
  eng = tr._engine('ed_vector')
  eng.set_params(vec); eng.set_configs(cfg); eng.set_bonds(BONDS, 1.0, 1.0)
  got = eng.projected_energy(perms, flips, chi)
  eloc, d_eloc = _eloc_reference('ed_vector', vec, psi, cfg)
  _, (wb, web, eb) = _check('4 x 4 ground state', got, psi, eps, eloc, d_eloc, cfg, perms, flips, chi)
  alive = got['n_alive']
  assert alive == B
  target = np.zeros(len(labels)); target[s0] = alive
  print('  max |w_sum - target| / bound %.3g' % (np.abs(got['w_sum'] - target) / wb).max())
  assert (np.abs(got['w_sum'] - target) <= wb).all()
  # tests/test_gpu_edvec.py (_eloc_bound, as test_edvec_evaluation_of_the_exact_state takes it): the largest bound over the chains
  tol = d_eloc.max()
  print('  |we_sum[s0] - E0 n_alive| = %.3g (n_alive x tolerance %.3g)' % (abs(got['we_sum'][s0] - e0 * alive), alive * tol))
  assert abs(got['we_sum'][s0] - e0 * alive) <= alive * tol
  # completeness: the characters sum to the identity's indicator
  assert abs(got['we_sum'].sum() - got['e_sum']) <= web.sum() + eb
  assert abs(got['w_sum'].sum() - alive) <= wb.sum()
  eng.close()


def _mixture_directory(path, n=8, mix=0.95):
  """A checkpoint directory (tools/make_ed_vector.py's) whose vector is mix v0 + sqrt(1 - mix^2) v1 of the n-site chain;
  -> (E0, E1, the vector in the Sz = 0 basis order, basis, Hamiltonian matrix)."""
  from tools import make_ed_vector as mk
  mk.main([path, '--lattice', 'chain', '--size', str(n)])
  basis = eo.sz0_configurations(n)
  hmat = pj.hamiltonian_matrix(basis, lattice.chain_bonds(n), 1.0, 1.0)
  w, v = np.linalg.eigh(hmat)
  state = mix * v[:, 0] + np.sqrt(1.0 - mix * mix) * v[:, 1]
  top, bot, length = eo.lin_tables(n)
  vec = np.zeros(length)
  vec[eo.index(basis, top, bot)] = state
  np.savetxt(path + '/ed_vector.txt', vec.astype(np.float32), fmt='%.9g')
  np.savez(path + '/model_prior_0_epochs.npz', **{'full_vector/ed_vector': vec.astype(np.float32)})
  return w[0], w[1], state, basis, hmat


def test_the_sampled_mixture_resolves_both_sectors(monkeypatch, tmp_path):
  """0.95 v0 + sqrt(1 - 0.95^2) v1 of the 8-site chain, sampled: 1,024 chains, 16 samples, 2 sweeps apart, 50 sweeps of
  equilibration, through ProjectedEnergyEvaluator (the driver's evaluate).  The caps on the errors are about 3.5 x the
  ideal 0.231 / sqrt(16384) and 2.14 / sqrt(16384) of independent chains (the margin is for autocorrelation at 2 sweeps);
  with them 5 errors stay below the distances 0.051 and 0.47 between the sector energies and the unprojected energy."""
  from cgs_vmc_amd import run_projected_energy_evaluation as rp, session, wavefunctions
  monkeypatch.setenv('CGS_VMC_SEED', '20241019')
  monkeypatch.setenv('CGS_VMC_CONFIG_SEED', '5')
  d = str(tmp_path / 'mix')
  e0, e1, state, basis, hmat = _mixture_directory(d)
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  flags = rp.cli_common.parser_from_table(rp.__doc__, rp.FLAG_TABLE).parse_args(
      ['--checkpoint_dir', d, '--spin_flip', '--hparams',
       'batch_size=1024,num_evaluation_samples=16,num_monte_carlo_sweeps=2,num_equilibration_sweeps=50'])
  _, _, labels, out = rp.evaluate(flags)
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  a, b = labels.index('q0+'), labels.index('q4-')
  plain = float(state @ hmat @ state)
  assert abs(plain - (-3.600133)) < 1e-6 and abs(e0 - (-3.651093)) < 1e-6 and abs(e1 - (-3.128419)) < 1e-6
  print('mixture: E(0,+) %.6f +- %.4f (E0 %.6f), E(4,-) %.5f +- %.4f (E1 %.6f), weights %.4f +- %.4f, %.4f +- %.4f, plain %.5f +- %.4f'
        % (out['energy'][a], out['energy_err'][a], e0, out['energy'][b], out['energy_err'][b], e1, out['weight'][a],
           out['weight_err'][a], out['weight'][b], out['weight_err'][b], out['plain_energy'], out['plain_energy_err']))
  assert out['samples'].shape == (16, 2 * len(labels) + 2) and (out['samples'][:, -1] == 1024).all()
  assert 0 < out['energy_err'][a] <= 0.006 and 0 < out['energy_err'][b] <= 0.06
  assert abs(out['energy'][a] - e0) <= 5 * out['energy_err'][a]
  assert abs(out['energy'][b] - e1) <= 5 * out['energy_err'][b]
  assert abs(out['weight'][a] - 0.9025) <= 5 * out['weight_err'][a]
  assert abs(out['weight'][b] - 0.0975) <= 5 * out['weight_err'][b]
  assert abs(out['plain_energy'] - plain) <= 5 * out['plain_energy_err']


def test_72_sites_144_ops_74_sectors_and_200_chains_go_past_one_wavefront_and_one_tile():
  """72-site chain, the 72 translations with and without the flip, every sector of the lattice (37 momentum classes x 2
  parities: five sector tiles), 200 chains: no multiple of 64, one partly filled block of k_proj_accum."""
  from cgs_vmc_amd.engine import VmcEngine
  n, b = 72, 200
  theta = vo.init_params(n, H, 2, np.random.default_rng(3))
  psi = lambda c: vo.fc_psi(theta, c, H, 2, dtype=np.float64)
  # tests/test_gpu_engine.py (test_amplitude_matches_oracle): |dlogit| <= 2e-5 max(1, |logit|)
  eps = lambda c: 2e-5 * np.maximum(1.0, np.abs(vo.fc_logit(theta, c, H, 2, dtype=np.float64)))
  labels, perms, flips, chi = _translation_sectors(n, 1)
  assert len(perms) == 144 and len(labels) == 74
  bonds = lattice.chain_bonds(n)
  cfg = tr._cfg(8, b=b, n=n)
  eng = VmcEngine(n, b, 2, H, seed=2024)
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(bonds, 1.0, 1.0)
  got = eng.projected_energy(perms, flips, chi)
  eloc, d_eloc = _eloc_reference('fully_connected', theta, psi, cfg, bonds)
  ref, (wb, web, eb) = _check('72 sites, 144 ops, 74 sectors', got, psi, eps, eloc, d_eloc, cfg, perms, flips, chi)
  assert (np.abs(ref['w_sum']) > 1e-2).sum() > len(labels) // 2      # a random network lives in no single sector
  assert abs(got['we_sum'].sum() - got['e_sum']) <= web.sum() + eb
  assert abs(got['w_sum'].sum() - b) <= wb.sum()
  _same(eng.projected_energy(perms, flips, chi, ops_per_pass=50), got)
  eng.close()


def _refused(eng, perms, flips, chi, n_ops=None, n_sectors=None, null_chi=False):
  """The C entry itself on arguments the Python side would not pass on: the return code and the ctx's message."""
  perms = np.ascontiguousarray(perms, np.int32)
  chi = np.ascontiguousarray(np.asarray(chi, np.float64).reshape(-1, len(perms)))
  fn = eng._lib.vmc_projected_energy
  fp = None if flips is None else np.ascontiguousarray(flips, np.uint8).ctypes.data_as(fn.argtypes[4])
  out = np.full(2 * len(chi) + 1, np.nan)
  alive = np.array([-7], np.int64)
  dp = fn.argtypes[6]
  rc = fn(eng._ctx, 0, len(perms) if n_ops is None else n_ops, perms.ctypes.data_as(fn.argtypes[3]), fp,
          len(chi) if n_sectors is None else n_sectors, None if null_chi else chi.ctypes.data_as(dp), 0,
          out[:len(chi)].ctypes.data_as(dp), out[len(chi):2 * len(chi)].ctypes.data_as(dp), out[2 * len(chi):].ctypes.data_as(dp),
          alive.ctypes.data_as(fn.argtypes[11]))
  assert np.isnan(out).all() and alive[0] == -7          # a refused call writes nothing
  return rc, eng._lib.vmc_last_error(eng._ctx).decode()


BAD = PERMS.copy()
BAD[3, 9] = BAD[3, 2]                                    # op 3 names a site twice
NO_SYMMETRY = PERMS.copy()
NO_SYMMETRY[3] = np.random.default_rng(12).permutation(N)      # op 3 is a bijection, but no symmetry of the torus


def _siblings(eng):
  pairs = lattice.all_pairs(N)[:9]
  return (np.stack(eng.pair_correlations(pairs)), np.stack(eng.renyi2_swap(tr.REGIONS[:4])),
          np.concatenate(eng.dimer_correlations(BONDS[:5], [(0, 1), (2, 4)])), eng.symmetry_expectations(PERMS, FLIPS))


def test_a_measurement_moves_nothing_else():
  theta, _, _ = tr._family('fully_connected')

  def prepared():
    eng = tr._engine()
    eng.set_params(theta); eng.set_configs(tr._cfg(6)); eng.set_bonds(BONDS, 1.0, 1.0)
    eng.mc_steps(3 * N)
    eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.mc_steps(N)                                      # straight from the sampler's caches into a measurement
    return eng
  eng, twin = prepared(), prepared()
  first = eng.projected_energy(PERMS, FLIPS, CHI)
  before = _siblings(eng)
  _same(eng.projected_energy(PERMS, FLIPS, CHI, ops_per_pass=3), first)
  assert _refused(eng, BAD, FLIPS, CHI)[0] == _hip.VMC_ERR_INVALID
  assert _refused(eng, NO_SYMMETRY, FLIPS, CHI)[0] == _hip.VMC_ERR_INVALID
  for x, y in zip(before, _siblings(eng)):              # each of the four siblings: equal bits before and after
    np.testing.assert_array_equal(x, y)
  np.testing.assert_array_equal(eng.get_configs(), twin.get_configs())
  assert eng.step_counter == twin.step_counter
  np.testing.assert_array_equal(eng.get_accumulators(), twin.get_accumulators())
  for x, y in zip(eng.local_energy_terms(), twin.local_energy_terms()):      # the Hamiltonian's bond set answers as before
    np.testing.assert_array_equal(x, y)
  twin.local_energy()                                    # the one exception: what a local-energy call leaves behind
  assert eng.last_connected_rows() == twin.last_connected_rows() > 0
  for e in (eng, twin):
    e.mc_steps(N)
  eng.projected_energy(PERMS, FLIPS, CHI)
  np.testing.assert_array_equal(eng.local_energy()[0], twin.local_energy()[0])
  for e in (eng, twin):
    e.mc_steps(N)
  np.testing.assert_array_equal(eng.get_configs(), twin.get_configs())
  eng.close(); twin.close()
  # two training epochs with and without a measurement between them: the same parameters
  params = []
  for measure in (False, True):
    eng = tr._engine(b=64, seed=77)
    eng.set_params(theta); eng.set_configs(tr._cfg(7, b=64)); eng.set_bonds(BONDS, 1.0, 1.0)
    for epoch in range(2):
      eng.epoch_energy_gradient(2 * N, 3, N, 1e10)
      eng.apply_adam(_hip.VMC_MODE_ENERGY_GRADIENT, 1e-2)
      if measure and epoch == 0:
        eng.projected_energy(PERMS, FLIPS, CHI, ops_per_pass=5)
        assert _refused(eng, NO_SYMMETRY, FLIPS, CHI)[0] == _hip.VMC_ERR_INVALID
    params.append((eng.get_params(), eng.get_configs(), eng.step_counter))
    eng.close()
  for x, y in zip(*params):
    np.testing.assert_array_equal(x, y)


def test_refusals():
  from cgs_vmc_amd.engine import VmcEngine
  theta, psi, eps = tr._family('fully_connected')
  cfg = tr._cfg(9)
  eng = tr._engine()
  eng.set_params(theta); eng.set_configs(cfg)
  rc, msg = _refused(eng, PERMS, FLIPS, CHI)
  assert rc == _hip.VMC_ERR_STATE and 'vmc_set_bonds' in msg           # no Hamiltonian to be a symmetry of
  eng.set_bonds(BONDS, 1.0, 1.0)
  eloc, d_eloc = _eloc_reference('fully_connected', theta, psi, cfg)

  def still_measures(tag):
    _check('after ' + tag, eng.projected_energy(PERMS, FLIPS, CHI), psi, eps, eloc, d_eloc, cfg, PERMS, FLIPS, CHI)
  still_measures('the missing bonds')
  rc, msg = _refused(eng, NO_SYMMETRY, FLIPS, CHI)
  assert rc == _hip.VMC_ERR_INVALID and msg.startswith('op 3 is no symmetry of the Hamiltonian: bond ') and ') goes to (' in msg, msg
  with pytest.raises(ValueError, match='op 3 is no symmetry'):
    eng.projected_energy(NO_SYMMETRY, FLIPS, CHI)
  still_measures('an op that is no symmetry')
  rc, msg = _refused(eng, BAD, FLIPS, CHI)
  assert rc == _hip.VMC_ERR_INVALID and 'op 3: entry 9' in msg, msg
  with pytest.raises(ValueError, match='op 3'):
    eng.projected_energy(BAD, FLIPS, CHI)
  still_measures('a non-bijection')
  assert _refused(eng, PERMS, FLIPS, CHI, null_chi=True)[0] == _hip.VMC_ERR_INVALID
  nan = CHI.copy(); nan[2, 4] = np.nan
  rc, msg = _refused(eng, PERMS, FLIPS, nan)
  assert rc == _hip.VMC_ERR_INVALID and 'sector 2' in msg and 'op 4' in msg, msg
  inf = CHI.copy(); inf[5, 0] = np.inf
  assert _refused(eng, PERMS, FLIPS, inf)[0] == _hip.VMC_ERR_INVALID
  with pytest.raises(ValueError, match='sector 2'):
    eng.projected_energy(PERMS, FLIPS, nan)
  still_measures('NULL and NaN characters')
  assert _refused(eng, PERMS, FLIPS, CHI, n_sectors=0)[0] == _hip.VMC_ERR_INVALID
  assert _refused(eng, PERMS, FLIPS, CHI, n_ops=0)[0] == _hip.VMC_ERR_INVALID
  rc, msg = _refused(eng, PERMS, FLIPS, CHI, n_sectors=(1 << 26) // B + 1)      # (refused before the characters are read)
  assert rc == _hip.VMC_ERR_UNSUPPORTED and 'accumulator budget' in msg, msg
  with pytest.raises(ValueError):
    eng.projected_energy(PERMS, FLIPS, CHI[:0])
  with pytest.raises(ValueError):
    eng.projected_energy(PERMS, FLIPS, CHI[:, :5])                   # characters for five of the seven ops
  with pytest.raises(ValueError):
    eng.projected_energy(PERMS, FLIPS, CHI, which=2)
  with pytest.raises(ValueError):
    eng.projected_energy(PERMS, FLIPS, CHI, ops_per_pass=-1)
  still_measures('no sector, no op, a bad which and a negative ops_per_pass')
  eng.set_bonds(BONDS, [1.0] * 7 + [0.5] + [1.0] * (len(BONDS) - 8), 1.0)      # one bond's j_x changed: T(1,0) is no symmetry
  rc, msg = _refused(eng, PERMS, FLIPS, CHI)
  assert rc == _hip.VMC_ERR_INVALID and msg.startswith('op 1 is no symmetry'), msg
  eng.projected_energy(PERMS[[0, 5]], FLIPS[[0, 5]], CHI[:, [0, 5]])           # the identity and the flip still are
  eng.set_bonds(BONDS, 1.0, 1.0)
  still_measures('a Hamiltonian the ops are no symmetries of')
  eng.close()
  cos = VmcEngine(N, B, 2, H, output_activation='cos', seed=2024)
  cos.set_params(theta); cos.set_configs(cfg); cos.set_bonds(BONDS, 1.0, 1.0)
  with pytest.raises(NotImplementedError, match='exp output'):
    cos.projected_energy(PERMS, FLIPS, CHI)
  cos.close()
  spec = dict(ansatz='fully_connected', num_layers=1, layer_size=H, nonlinearity='relu', output_activation='exp')
  prod = VmcEngine(N, B, 0, 0, ansatz='prod', children=[spec, dict(spec, ansatz='rbm')], seed=2024)
  with pytest.raises(NotImplementedError, match='product ctx'):
    prod.projected_energy(PERMS, FLIPS, CHI)
  with pytest.raises(_hip.ComposedFactorError):
    prod.children[0].projected_energy(PERMS, FLIPS, CHI)
  prod.close()


def test_cli_on_a_tiny_checkpoint_directory_writes_sector_energies(monkeypatch, tmp_path):
  """The 0.8 / 0.6 mixture of the two lowest states of the 6-site chain: two sectors carry weight, the others are noise."""
  from cgs_vmc_amd import run_projected_energy_evaluation as rp, session, wavefunctions
  monkeypatch.setenv('CGS_VMC_SEED', '20241019')
  monkeypatch.setenv('CGS_VMC_CONFIG_SEED', '5')
  d, out = str(tmp_path / 'ed'), str(tmp_path / 'out')
  _mixture_directory(d, n=6, mix=0.8)
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  result, written = rp.main(['--checkpoint_dir', d, '--output_dir', out, '--spin_flip', '--hparams',
                             'batch_size=32,num_evaluation_samples=3,num_monte_carlo_sweeps=2'])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  assert written == [out + '/sector_energies.txt']
  labels, chi = lattice.sector_characters(6, 1, True)
  np.testing.assert_array_equal(result['characters'], chi)
  np.testing.assert_array_equal(result['perms'], np.concatenate([lattice.translations(6)] * 2))
  lines = [l.split() for l in open(written[0]) if not l.startswith('#')]
  assert [l[0] for l in lines] == labels and len(labels) == 8
  table = np.array([[float(x) for x in l[1:5]] for l in lines])
  want = np.stack([result['weight'], result['weight_err'], result['energy'], result['energy_err']], axis=1)
  np.testing.assert_allclose(table, want, rtol=1e-9, equal_nan=True)
  flags = [len(l) == 6 and l[5] == 'unresolved' for l in lines]
  assert all(len(l) in (5, 6) for l in lines)
  assert flags == (np.abs(result['weight']) < 3 * result['weight_err']).tolist()
  tail = [l for l in open(written[0]) if l.startswith('# unprojected energy')]
  assert len(tail) == 1 and abs(float(tail[0].split()[3]) - result['plain_energy']) <= 1e-9 * abs(result['plain_energy'])

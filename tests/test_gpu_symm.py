"""GPU: symmetry expectation values (vmc_symmetry_expectations: csrc/vmc_api_measure.hip + symm.hip; SymmetryEvaluator;
run_symmetry_evaluation) against the fp64 oracle tests/symm_oracle.py.

Bound.  A chain's term is exp of the difference of two fp32 logs ln|psi| (the permuted row minus the chain), formed in
fp64.  With eps(r) the bound the family's own amplitude / logit parity test applies to ln|psi| of row r (the constants of
`_family` in tests/test_gpu_renyi.py, each next to the file it is taken from; imported here), the term is within
|term_ref| (exp(eps(row) + eps(x)) - 1) of the oracle's, and an fp64 fold of B terms in any fixed order adds
B 2^-53 sum |term_ref|:
  |ratio_sum_k - ref_k| <= sum_c |t_c| (exp(eps(row_{k,c}) + eps(x_c)) - 1) + B 2^-53 sum_c |t_c|
No case is left out of the comparison; rows with psi = 0 are 0 on both sides.
"""
import functools

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from cgs_vmc_amd import lattice
from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo
from tests import symm_oracle as so
from tests import test_gpu_renyi as tr

pytestmark = pytest.mark.gpu
N, H, B = tr.N, tr.H, tr.B                  # 4 x 4 torus, H = 32, 40 chains: no multiple of the 8- or 16-chain tiles
FAMILIES = tr.FAMILIES


def _ops16():
  """identity; T(1,0), T(0,1), rot90, mirror_x; the flip alone and T(1,1) + flip; one random permutation that is no
  lattice symmetry, so that the convolutional terms are not all 1."""
  t = lattice.translations(4, 4)
  labels, group = lattice.point_group(4, 4)
  rand = np.random.default_rng(12).permutation(N).astype(np.int32)
  perms = np.stack([t[0], t[1], t[4], group[labels.index('rot90')], group[labels.index('mirror_x')], t[0], t[5], rand])
  flips = np.array([0, 0, 0, 0, 0, 1, 1, 0], np.uint8)
  return perms, flips


PERMS, FLIPS = _ops16()


def _reference(psi, eps, cfg, perms, flips):
  """(ratio_sum, bound) [n_ops] from the oracle."""
  cfg = np.asarray(cfg, np.float32)
  terms = so.terms(psi, cfg, perms, flips)
  e_own = eps(cfg)
  bound = np.zeros(len(perms))
  for k, (perm, flip) in enumerate(zip(perms, flips)):
    a = np.abs(terms[k])
    bound[k] = (a * np.expm1(eps(so.rows(cfg, perm, flip)) + e_own)).sum() + len(cfg) * 2.0 ** -53 * a.sum()
  return terms.sum(1), bound


def _check(tag, got, ref, bound):
  err = np.abs(got - ref)
  with np.errstate(divide='ignore', invalid='ignore'):
    rel = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
  k = int(np.argmax(rel))
  print('%s: worst error / bound %.3g (op %d: error %.3g, bound %.3g, value %.9g)' % (tag, rel[k], k, err[k], bound[k], ref[k]))
  assert np.isfinite(got).all()
  assert (err <= bound).all(), (tag, k, err[k], bound[k])


@pytest.mark.parametrize('ansatz', FAMILIES)
def test_ratio_sums_match_the_fp64_oracle(ansatz):
  theta, psi, eps = tr._family(ansatz)
  cfg = tr._cfg(2)
  assert (cfg.sum(1) == 0).all()
  eng = tr._engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg)
  got = eng.symmetry_expectations(PERMS, FLIPS)
  ref, bound = _reference(psi, eps, cfg, PERMS, FLIPS)
  _check(ansatz, got, ref, bound)
  alive = float((psi(cfg) != 0).sum())
  assert abs(got[0] - alive) <= bound[0]                    # the identity: 1 per chain whose own amplitude does not vanish
  if ansatz == 'ed_vector':
    dead = (so.terms(psi, cfg, PERMS, FLIPS) == 0).sum()
    assert alive < B or dead > 0                            # the zeroed entries are met
  else:
    assert alive == B
  if ansatz == 'conv_2d':                                   # translation invariant by construction; the random op is not
    assert abs(ref[1] - B) < 1e-9 and abs(ref[2] - B) < 1e-9 and abs(ref[-1] - B) > 1e-3
  # no flips is flip = None; the supervisor's parameter set measures through the same entry
  np.testing.assert_array_equal(eng.symmetry_expectations(PERMS[:5]), got[:5])
  eng.set_params(theta, _hip.VMC_OMEGA)
  np.testing.assert_array_equal(eng.symmetry_expectations(PERMS, FLIPS, which=_hip.VMC_OMEGA), got)
  eng.close()


def test_pass_splits_and_repeats_are_bit_identical():
  theta, psi, eps = tr._family('fully_connected')
  eng = tr._engine()
  eng.set_params(theta); eng.set_configs(tr._cfg(7))
  base = eng.symmetry_expectations(PERMS, FLIPS)
  for per in (1, 3, 0):
    for _ in range(2):
      np.testing.assert_array_equal(eng.symmetry_expectations(PERMS, FLIPS, ops_per_pass=per), base,
                                    err_msg='ops_per_pass=%d' % per)
  # ... nor on which other ops are in the list, or where
  pick = np.array([6, 2, 7, 0])
  np.testing.assert_array_equal(eng.symmetry_expectations(PERMS[pick], FLIPS[pick], ops_per_pass=3), base[pick])
  eng.close()


def test_72_sites_and_144_ops_go_past_one_wavefront_and_one_fold_block():
  """72-site chain: more than 64 sites per row (the lanes of k_symm_rows wrap); the 72 translations with and without the
  flip: 144 ops, more than two blocks of 64; 24 chains: fewer than the 64 lanes of k_symm_fold."""
  from cgs_vmc_amd.engine import VmcEngine
  n, b = 72, 24
  theta = vo.init_params(n, H, 2, np.random.default_rng(3))
  psi = lambda c: vo.fc_psi(theta, c, H, 2, dtype=np.float64)
  # tests/test_gpu_engine.py (test_amplitude_matches_oracle): |dlogit| <= 2e-5 max(1, |logit|)
  eps = lambda c: 2e-5 * np.maximum(1.0, np.abs(vo.fc_logit(theta, c, H, 2, dtype=np.float64)))
  t = lattice.translations(n)
  perms = np.concatenate([t, t])
  flips = np.repeat([0, 1], n).astype(np.uint8)
  cfg = tr._cfg(8, b=b, n=n)
  eng = VmcEngine(n, b, 2, H, seed=2024)
  eng.set_params(theta); eng.set_configs(cfg)
  got = eng.symmetry_expectations(perms, flips)
  ref, bound = _reference(psi, eps, cfg, perms, flips)
  _check('72 sites, 144 ops', got, ref, bound)
  assert np.abs(ref - b).max() > 1e-2                       # a random network is no eigenstate of anything
  np.testing.assert_array_equal(eng.symmetry_expectations(perms, flips, ops_per_pass=50), got)
  eng.close()


@functools.lru_cache(maxsize=None)
def _torus_ground_state():
  return eo.vector_from_ed(N, tr.BONDS, 1.0, 1.0)


def test_exact_ground_states_give_their_characters_signs_included():
  """ed_vector loaded with an exact ground state: psi(g x) = chi(g) psi(x) on every configuration, so ratio_sum / B is the
  character with no Monte-Carlo error, whatever the chains.  Each value within 1e-5: two fp32 logarithms of magnitude
  below 8 carry at most 2 x 2^-21, the fp32 rounding of the two entries adds 2 x 2^-24; about a factor 4 is left."""
  n6, b = 6, 40
  _, vec, top, bot = eo.vector_from_ed(n6, lattice.chain_bonds(n6), 1.0, 1.0)
  assert (vec != 0).all() and np.abs(np.log(np.abs(vec))).max() < 8
  t = lattice.translations(n6)
  perms = np.stack([t[0], t[1], t[2], lattice.point_group(n6)[1][1], t[0]])
  flips = np.array([0, 0, 0, 0, 1], np.uint8)
  eng = tr._engine('ed_vector', n=n6, b=b)
  eng.set_params(vec.astype(np.float32)); eng.set_configs(tr._cfg(4, b=b, n=n6))
  got = eng.symmetry_expectations(perms, flips) / b
  print('6-site chain, j_x = +1: (id, T1, T2, mirror, flip) =', got)
  assert np.abs(got - [1, -1, 1, 1, -1]).max() < 1e-5
  eng.close()
  _, vec, top, bot = _torus_ground_state()
  assert np.abs(np.log(np.abs(vec[vec != 0]))).max() < 8
  labels, group = lattice.point_group(4, 4)
  t = lattice.translations(4, 4)
  perms = np.stack([t[1], group[labels.index('rot90')], t[0]])
  flips = np.array([0, 0, 1], np.uint8)
  cfg = tr._cfg(4)
  assert (eo.amplitude(vec.astype(np.float32), cfg, top, bot) != 0).all()
  eng = tr._engine('ed_vector')
  eng.set_params(vec.astype(np.float32)); eng.set_configs(cfg)
  got = eng.symmetry_expectations(perms, flips) / B
  print('4 x 4 torus, j_x = +1: (T(1,0), rot90, flip) =', got)
  assert np.abs(got - 1.0).max() < 1e-5
  eng.close()


def test_evaluator_gives_momentum_zero_on_an_exact_network_state(monkeypatch):
  """exact_fc_eigenstate on the 8-site chain (2 x 128 units, j_x = -1): the network IS the ground state on the whole
  sector -- k = 0, even under the mirror and the flip -- so every value is 1 whatever the chains, within
  expm1(2 eps) for the dense family's eps = 2e-5 max(1, |logit|) (tests/test_gpu_engine.py), taken at the sector's
  largest |logit|."""
  from cgs_vmc_amd import evaluation, session, utils, wavefunctions
  from tests.exact_states import exact_fc_eigenstate
  n, h, layers = 8, 128, 2
  monkeypatch.setenv('CGS_VMC_SEED', '77')
  monkeypatch.setenv('CGS_VMC_CONFIG_SEED', '5')
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  theta, _, cfgs, _ = exact_fc_eigenstate(n, lattice.chain_bonds(n), h, layers)
  eps = 2e-5 * max(1.0, np.abs(vo.fc_logit(theta, cfgs, h, layers, dtype=np.float64)).max())
  figure = np.expm1(2 * eps)
  hp = utils.create_hparams(wavefunction_type='fully_connected', num_sites=n, num_fc_layers=layers, fc_layer_size=h,
                            batch_size=48, num_equilibration_sweeps=5, num_monte_carlo_sweeps=1, num_evaluation_samples=2)
  wf = wavefunctions.build_wavefunction(hp)
  perms = np.concatenate([lattice.translations(n), lattice.point_group(n)[1][1:], np.arange(n)[None, :]])
  flips = np.array([0] * 9 + [1], np.uint8)
  ev = evaluation.SymmetryEvaluator()
  eops = ev.build_eval_ops(wavefunction=wf, operator=(perms, flips), hparams=hp, shared_resources={})
  sess = session.Session()
  sess.run(session.global_variables_initializer())
  wf._set_theta(theta)
  out = ev.run_evaluation(eops, sess, hp, epoch_num=0)
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  assert out['samples'].shape == (2, 10) and ev.acceptance_count > 0
  np.testing.assert_array_equal(out['perms'], perms); np.testing.assert_array_equal(out['flips'], flips)
  weights = lattice.momentum_weights(out['value'][:n], n)
  print('exact 8-site state: max |value - 1| %.3g, max value_err %.3g, max |weight - delta| %.3g (figure %.3g)'
        % (np.abs(out['value'] - 1).max(), out['value_err'].max(), np.abs(weights - np.eye(n)[0]).max(), figure))
  assert np.abs(out['value'] - 1.0).max() <= figure
  assert np.abs(weights - np.eye(n)[0]).max() <= figure
  assert out['value_err'].max() < figure


def _state(eng):
  return (eng.local_energy()[0], eng.get_configs(), eng.step_counter, eng.get_accumulators())


def _refused(eng, perms, flips=None, n_ops=None):
  """The C entry itself on ops the Python side would not pass on: the return code and the ctx's message."""
  perms = np.ascontiguousarray(perms, np.int32)
  fn = eng._lib.vmc_symmetry_expectations
  fp = None if flips is None else np.ascontiguousarray(flips, np.uint8).ctypes.data_as(fn.argtypes[4])
  out = np.full(max(len(perms), 1), np.nan)
  rc = fn(eng._ctx, 0, len(perms) if n_ops is None else n_ops, perms.ctypes.data_as(fn.argtypes[3]), fp, 0,
          out.ctypes.data_as(fn.argtypes[6]))
  assert np.isnan(out).all()                             # a refused call writes nothing
  return rc, eng._lib.vmc_last_error(eng._ctx).decode()


BAD = PERMS.copy()
BAD[3, 9] = BAD[3, 2]                                    # op 3 names a site twice


def test_a_measurement_moves_nothing_else():
  theta, _, _ = tr._family('fully_connected')
  eng = tr._engine()
  eng.set_params(theta); eng.set_configs(tr._cfg(6)); eng.set_bonds(tr.BONDS, 1.0, 1.0)
  eng.mc_steps(3 * N)
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  before = _state(eng)
  terms = eng.local_energy_terms()
  eng.symmetry_expectations(PERMS, FLIPS); eng.symmetry_expectations(PERMS, FLIPS, ops_per_pass=3)
  assert _refused(eng, BAD, FLIPS)[0] == _hip.VMC_ERR_INVALID
  after = _state(eng)
  for x, y in zip(before, after):
    np.testing.assert_array_equal(x, y)
  for x, y in zip(terms, eng.local_energy_terms()):    # the Hamiltonian's bond set answers as before
    np.testing.assert_array_equal(x, y)
  eng.mc_steps(N)                                      # straight from the sampler's caches into a measurement
  eloc = eng.local_energy()[0]
  eng.mc_steps(N); chains = eng.get_configs()
  eng.close()
  for refuse in (False, True):
    eng = tr._engine()
    eng.set_params(theta); eng.set_configs(tr._cfg(6)); eng.set_bonds(tr.BONDS, 1.0, 1.0)
    eng.mc_steps(3 * N)
    eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.mc_steps(N)
    if refuse:
      assert _refused(eng, BAD, FLIPS)[0] == _hip.VMC_ERR_INVALID
    else:
      eng.symmetry_expectations(PERMS, FLIPS)
    np.testing.assert_array_equal(eng.local_energy()[0], eloc)
    eng.mc_steps(N)
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
        eng.symmetry_expectations(PERMS, FLIPS, ops_per_pass=5)
        assert _refused(eng, BAD, FLIPS)[0] == _hip.VMC_ERR_INVALID
    params.append((eng.get_params(), eng.get_configs(), eng.step_counter))
    eng.close()
  for x, y in zip(*params):
    np.testing.assert_array_equal(x, y)


def test_refusals():
  from cgs_vmc_amd.engine import VmcEngine
  theta, psi, eps = tr._family('fully_connected')
  cfg = tr._cfg(9)
  eng = tr._engine()
  eng.set_configs(cfg)
  with pytest.raises(_hip.HipLibraryError, match='parameters not set'):
    eng.symmetry_expectations(PERMS, FLIPS)
  eng.set_params(theta)
  ref, bound = _reference(psi, eps, cfg, PERMS, FLIPS)

  def still_measures(tag):
    _check('after ' + tag, eng.symmetry_expectations(PERMS, FLIPS), ref, bound)
  still_measures('the missing parameters')
  site_n = PERMS.copy(); site_n[6, 15] = N
  negative = PERMS.copy(); negative[0, 0] = -1
  flip2 = FLIPS.copy(); flip2[5] = 2
  # the Python side refuses without a library call, the C entry refuses by itself and names the op and the entry
  for tag, perms, flips, names in (('a non-bijective permutation', BAD, FLIPS, 'op 3: entry 9'),
                                   ('a site equal to N', site_n, FLIPS, 'op 6: entry 15'),
                                   ('a negative site', negative, FLIPS, 'op 0: entry 0'),
                                   ('a flip of 2', PERMS, flip2, 'op 5: flip')):
    with pytest.raises(ValueError, match=names.split(':')[0]):
      eng.symmetry_expectations(perms, flips)
    rc, msg = _refused(eng, perms, flips)
    assert rc == _hip.VMC_ERR_INVALID and names in msg, (tag, rc, msg)
    still_measures(tag)
  with pytest.raises(ValueError):
    eng.symmetry_expectations(np.zeros((0, N), np.int32))          # zero ops
  with pytest.raises(ValueError):
    eng.symmetry_expectations([])
  assert _refused(eng, PERMS, FLIPS, n_ops=0)[0] == _hip.VMC_ERR_INVALID
  fn = eng._lib.vmc_symmetry_expectations
  assert fn(eng._ctx, 0, 1, None, None, 0, None) == _hip.VMC_ERR_INVALID
  still_measures('zero ops')
  with pytest.raises(ValueError):
    eng.symmetry_expectations(PERMS[:, :N - 1])                    # a wrong length
  with pytest.raises(ValueError):
    eng.symmetry_expectations(PERMS, FLIPS, which=2)
  with pytest.raises(ValueError):
    eng.symmetry_expectations(PERMS, FLIPS, ops_per_pass=-1)
  still_measures('a bad which and a negative ops_per_pass')
  eng.close()
  cos = VmcEngine(N, B, 2, H, output_activation='cos', seed=2024)
  cos.set_params(theta); cos.set_configs(cfg)
  with pytest.raises(NotImplementedError, match='exp output'):
    cos.symmetry_expectations(PERMS, FLIPS)
  cos.close()
  spec = dict(ansatz='fully_connected', num_layers=1, layer_size=H, nonlinearity='relu', output_activation='exp')
  prod = VmcEngine(N, B, 0, 0, ansatz='prod', children=[spec, dict(spec, ansatz='rbm')], seed=2024)
  with pytest.raises(NotImplementedError, match='product ctx'):
    prod.symmetry_expectations(PERMS, FLIPS)
  with pytest.raises(_hip.ComposedFactorError):
    prod.children[0].symmetry_expectations(PERMS, FLIPS)
  prod.close()


def test_cli_on_a_tiny_checkpoint_directory_writes_both_files(monkeypatch, tmp_path):
  """The 6-site chain's exact ground state (tools/make_ed_vector.py, j_x = +1): momentum pi, even mirror, odd flip."""
  from cgs_vmc_amd import run_symmetry_evaluation as rs, session, wavefunctions
  from tools import make_ed_vector as mk
  monkeypatch.setenv('CGS_VMC_SEED', '20241018')
  monkeypatch.setenv('CGS_VMC_CONFIG_SEED', '5')
  d, out = str(tmp_path / 'ed'), str(tmp_path / 'out')
  mk.main([d, '--lattice', 'chain', '--size', '6'])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  result, written = rs.main(['--checkpoint_dir', d, '--output_dir', out, '--spin_flip', '--hparams',
                             'batch_size=32,num_evaluation_samples=3,num_monte_carlo_sweeps=2'])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  assert written == [out + '/symmetries.txt', out + '/momentum_weights.txt']
  labels, perms, flips = rs.default_ops(6, 1, True)
  np.testing.assert_array_equal(result['perms'], perms); np.testing.assert_array_equal(result['flips'], flips)
  lines = [l.split() for l in open(written[0]) if not l.startswith('#')]
  assert len(lines) == 14 and [l[0] for l in lines] == labels and [int(l[1]) for l in lines] == flips.tolist()
  values = np.array([float(l[2]) for l in lines])
  np.testing.assert_allclose(values, result['value'], rtol=1e-9)
  character = np.array([1, -1, 1, -1, 1, -1, 1])         # T(0) .. T(5), mirror; the flip multiplies by -1
  assert np.abs(values - np.concatenate([character, -character])).max() < 1e-5
  rows = np.loadtxt(written[1])
  assert rows.shape == (6, 3) and np.isfinite(rows).all()
  np.testing.assert_allclose(rows[:, 0], lattice.chain_momenta(6)[:, 0], rtol=1e-9)
  assert np.abs(rows[:, 1] - np.eye(6)[3]).max() < 1e-5                 # all the weight at q = pi

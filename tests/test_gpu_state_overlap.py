"""GPU: the overlap with the frozen parameter set (vmc_overlap) and the penalised accumulate / gradient / Adam / epoch
(VMC_MODE_PENALIZED_ENERGY) on every kernel path, against tests/overlap_cases.py fed with the amplitudes the engine itself
reports (the kernels read the same fp32 caches), against modes 0 and 1 of the library, and end to end on the 8-site chain.

Engines, parameters, chains and bonds are those of tests/golden/make_path_bits.py (N = 16 on the 4 x 4 torus, 64 chains);
omega = theta + 0.02 normal(seed 8), the perturbation of tests/test_gpu_engine.py.

Bounds.  d_c is formed from fp32 inputs by three fp64 subtractions in one order on both sides: log_scale and the chains
alive are compared with ==.  S1, S2 and the ratios differ from numpy's by the fp64 exponential and the summation order
alone: rtol 1e-9 (the rtol tests/test_gpu_symm.py gives fp64 host arithmetic).  Gradients: 2e-3 max|ref| + 1e-4 (2e-4 where
tests/test_gpu_engine.py says so), scalars 2e-4 max(1, |x|), Adam atol 2e-6 -- all from tests/test_gpu_engine.py."""
import importlib.util
import os

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import overlap_cases as oc

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
  spec = importlib.util.spec_from_file_location(name, path)
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


make_path_bits = _load('make_path_bits', os.path.join(_HERE, 'golden', 'make_path_bits.py'))
N, B = make_path_bits.N, make_path_bits.B
PRODUCT = 'prod_pbdg_fc'
CASES = [name for name in make_path_bits.CASES if name != PRODUCT]          # the 15 that are no product ctx
SIGNED_PATHS = (7, 8, 9)                                                    # pbdg, nnb, ed_vector
LAM = 1.5
MODE2 = _hip.VMC_MODE_PENALIZED_ENERGY


def _created(name):
  path, env = make_path_bits.CASES[name]
  saved = {k: os.environ.get(k) for k in env}
  os.environ.update(env)
  try:
    eng, theta = make_path_bits._make(name)
  finally:
    for k, v in saved.items():
      if v is None:
        del os.environ[k]
      else:
        os.environ[k] = v
  assert eng.kernel_path() == path
  return eng, theta


def _omega(theta):
  return theta + (0.02 * np.random.default_rng(8).standard_normal(theta.size)).astype(np.float32)


def _engine(name, frozen=True):
  """An engine of the case in the state make_path_bits.run_case starts from -- parameters, chains, the torus bonds -- and
  with `frozen` the perturbed parameters in the second set."""
  from tests import test_gpu_buffers as tb
  from tests import test_gpu_renyi as tr
  eng, theta = _created(name)
  eng.set_params(theta)
  eng.set_configs(tr._cfg(2, b=B))
  eng.set_bonds(tb.TORUS, 1.0, 1.0)
  if frozen:
    eng.set_params(_omega(theta), _hip.VMC_OMEGA)
  return eng, theta


def _dense(b, **kw):
  """The fully_connected case at another batch size."""
  from tests import test_gpu_buffers as tb
  from tests import test_gpu_renyi as tr
  eng, theta = tr._engine('fully_connected', b=b, **kw), tr._family('fully_connected')[0]
  eng.set_params(theta)
  eng.set_configs(tr._cfg(2, b=b))
  eng.set_bonds(tb.TORUS, 1.0, 1.0)
  eng.set_params(_omega(theta), _hip.VMC_OMEGA)
  return eng, theta


def _signs(eng):
  """(sign of psi, sign of omega) [B] on the chains of a signed type, else (None, None): read off the fp32 amplitudes the
  engine reports, so at exponent shifts that leave them inside fp32."""
  if eng.kernel_path() not in SIGNED_PATHS:
    return None, None
  return np.sign(eng.amplitude(which=_hip.VMC_PSI)[1]), np.sign(eng.amplitude(which=_hip.VMC_OMEGA)[1])


def _reference(eng, signs=None):
  """overlap_cases on the amplitudes the engine reports for its chains (`signs`: those of _signs, taken earlier)."""
  sp, so = _signs(eng) if signs is None else signs
  lp, lo = eng.amplitude(which=_hip.VMC_PSI)[0], eng.amplitude(which=_hip.VMC_OMEGA)[0]
  r = oc.ratios(lp, sp, eng.get_shift(_hip.VMC_PSI), lo, so, eng.get_shift(_hip.VMC_OMEGA))
  return r, oc.sums(r)


def _check_sums(tag, got, ref):
  print('%s: alive %d log_scale %r s1 %.17g (ref %.17g) s2 %.17g (ref %.17g) max ratio error %.3g' % (
      tag, got['alive'], got['log_scale'], got['s1'], ref['s1'], got['s2'], ref['s2'],
      np.abs(got['ratio'] - ref['ratio']).max()))
  assert got['alive'] == ref['alive']
  assert got['log_scale'] == ref['log_scale']
  np.testing.assert_allclose(got['s1'], ref['s1'], rtol=1e-9, atol=0)
  np.testing.assert_allclose(got['s2'], ref['s2'], rtol=1e-9, atol=0)
  np.testing.assert_allclose(got['ratio'], ref['ratio'], rtol=1e-9, atol=0)


def _words(x):
  a = np.ascontiguousarray(x)
  return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_words(a, b):
  return np.array_equal(_words(a), _words(b))


def _fidelity(v):
  return v['s1'] ** 2 / (v['alive'] * v['s2'])


def _grad_close(tag, got, ref, atol):
  err, tol = np.abs(got - ref).max(), 2e-3 * np.abs(ref).max() + atol
  print('%s: max error %.3g, bound %.3g' % (tag, err, tol))
  assert err <= tol, (tag, err, tol)


# ---- 1. the sums on every path

@pytest.mark.parametrize('name', CASES)
def test_sums_on_every_path(name):
  eng, theta = _engine(name)
  try:
    r, ref = _reference(eng)
    got = eng.overlap(per_chain=True)
    _check_sums(name, got, ref)
    assert 0 < got['alive'] <= B and got['s2'] > 0
    if name == 'ed_vector':
      # theta has exact zeros: chains on them are dead
      assert got['alive'] < B and (~r.alive).sum() == B - got['alive']
      assert (got['ratio'][~r.alive] == 0).all()
      # ... and the other way round phi vanishes there: a ratio of 0 exactly, the chain stays alive
      eng.set_params(_omega(theta), _hip.VMC_PSI)
      eng.set_params(theta, _hip.VMC_OMEGA)
      r2, ref2 = _reference(eng)
      got2 = eng.overlap(per_chain=True)
      _check_sums(name + ' (swapped)', got2, ref2)
      assert got2['alive'] == B and (r2.s == 0).sum() == B - got['alive']
      assert (got2['ratio'][r2.s == 0] == 0).all()
    assert not eng.overlap().keys() & {'ratio'}
  finally:
    eng.close()


# ---- 2. scale: the ratios themselves leave fp64 and fp32, the sums do not

@pytest.mark.parametrize('name', ['fully_connected', 'pbdg'])
def test_scale_of_the_frozen_state_moves_log_scale_alone(name):
  eng, _ = _engine(name)
  try:
    base = eng.overlap()
    shift = eng.get_shift(_hip.VMC_OMEGA)
    signs = _signs(eng)                                # (exp(logit - shift) leaves fp32 below: the signs do not move)
    for delta in (200.0, -200.0):                      # d_c ~ +200 / -200: exp(2 d) is beyond fp64 either way
      eng.set_shift(shift - delta, _hip.VMC_OMEGA)
      assert eng.get_shift(_hip.VMC_OMEGA) == shift - delta
      got = eng.overlap(per_chain=True)
      _check_sums('%s d %+g' % (name, delta), got, _reference(eng, signs)[1])
      assert np.isfinite([got['s1'], got['s2'], got['log_scale']]).all() and np.isfinite(got['ratio']).all()
      np.testing.assert_allclose(_fidelity(got), _fidelity(base), rtol=1e-9, atol=0)
      # log_scale is one fp64 subtraction at magnitude 200 on either side: it moves by delta to that rounding
      assert abs((got['log_scale'] - base['log_scale']) - delta) <= 256 * 2.0 ** -53
      assert abs(got['log_scale']) > 150
    eng.set_shift(shift, _hip.VMC_OMEGA)
    again = eng.overlap()
    assert again == base
  finally:
    eng.close()


# ---- 3. the tails of the fold

@pytest.mark.parametrize('b,chain_offset', [(1, 0), (5, 0), (63, 0), (65, 7), (1025, 0)])
def test_fold_tails(b, chain_offset):
  eng, _ = _dense(b, chain_offset=chain_offset)
  try:
    ref = _reference(eng)[1]
    first, second = eng.overlap(per_chain=True), eng.overlap(per_chain=True)
    _check_sums('B = %d' % b, first, ref)
    assert first['alive'] == b
    for k in ('s1', 's2', 'log_scale'):
      assert _same_words(np.float64(first[k]), np.float64(second[k])), k
    assert first['alive'] == second['alive'] and _same_words(first['ratio'], second['ratio'])
  finally:
    eng.close()


# ---- 4. identity

@pytest.mark.parametrize('name', ['fully_connected', 'pbdg'])
def test_identity_after_transfer_params(name):
  eng, _ = _engine(name, frozen=False)
  try:
    eng.transfer_params()
    got = eng.overlap(per_chain=True)
    assert got['s1'] == B and got['s2'] == B and got['alive'] == B and got['log_scale'] == 0.0
    assert (got['ratio'] == 1.0).all()
    # w = E_loc + lambda: a constant drops out of the covariance
    eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    ref = eng.get_gradient(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.reset_accumulators(); eng.accumulate(MODE2, 1.0)
    _grad_close(name, eng.get_gradient(MODE2), ref, 2e-4)
    tail = eng.get_accumulators()[-8:]
    assert tail[5] == 1.0 and tail[6] == 1.0
  finally:
    eng.close()


# ---- 5. linearity in the weights, every path

@pytest.mark.parametrize('name', CASES)
def test_accumulators_are_linear_in_the_weights(name):
  eng, _ = _engine(name)
  try:
    p = eng.num_params
    eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    acc0 = eng.get_accumulators().astype(np.float64)
    eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.0)       # weights: exactly r_c
    acc1 = eng.get_accumulators().astype(np.float64)
    eng.reset_accumulators(); eng.accumulate(MODE2, LAM)
    acc2 = eng.get_accumulators().astype(np.float64)
    assert (acc0[-3:] == 0).all() and (acc1[-3:] == 0).all()                              # slots 5 and 6 are mode 2's
    r, ref = _reference(eng)
    ov = eng.overlap()
    _grad_close(name + ' g1', acc2[:p], acc0[:p], 1e-4)
    coef = LAM * (ov['s1'] / ov['s2']) * np.exp(-ov['log_scale'])                         # r_c = exp(m) ratio_c
    _grad_close(name + ' g2', acc2[p:2 * p], acc0[p:2 * p] + coef * acc1[p:2 * p], 1e-4)
    eloc = eng.local_energy()[0]
    w = oc.weights(eloc, r, LAM).astype(np.float64)
    expect = [acc0[2 * p], float(B), w.sum(), float(B), 1.0, _fidelity(ref), 1.0, 0.0]
    print(name, 'scalars', acc2[-8:], 'expected', expect)
    for k, (got, want) in enumerate(zip(acc2[-8:], expect)):
      if not np.isfinite(want):                    # ed_vector: a dead chain's local energy is x / 0, on both sides
        assert not np.isfinite(got), k
      else:
        assert abs(got - want) <= 2e-4 * max(1.0, abs(want)), (k, got, want)
  finally:
    eng.close()


# ---- 6. the gradient formula and Adam

def test_gradient_formula_and_adam():
  eng, theta = _engine('fully_connected')
  try:
    p = eng.num_params
    eng.reset_accumulators()
    eng.accumulate(MODE2, LAM); eng.mc_steps(N); eng.accumulate(MODE2, LAM)
    acc = eng.get_accumulators().astype(np.float64)
    sc = acc[-8:]
    assert sc[1] == 2 * B and sc[3] == 2 * B and sc[4] == 2 and sc[6] == 2
    ref = oc.penalized_gradient(acc[:p], acc[p:2 * p], sc[2], (sc[3], sc[4]))
    got = eng.get_gradient(MODE2)
    # the kernel forms g2 / n - (r_total / r_count) g1 / n in fp32 from the same accumulators: a few roundings per term
    eps = np.finfo(np.float32).eps
    bound = 4 * eps * (np.abs(acc[p:2 * p] / sc[4]) + np.abs(sc[2] / sc[3] * acc[:p] / sc[4])) + 1e-30
    print('gradient: worst error / bound %.3g' % (np.abs(got - ref) / bound).max())
    assert (np.abs(got - ref) <= bound).all()
    th_ref = vo.adam_apply(vo.AdamState(p), theta, ref, 1e-3, 0.9, 0.99, 1e-8)
    energy = eng.apply_adam(MODE2, 1e-3, 0.9, 0.99, 1e-8)
    assert abs(energy - sc[0] / sc[1]) <= 2e-4 * max(1.0, abs(sc[0] / sc[1]))
    np.testing.assert_allclose(eng.get_params(), th_ref, rtol=0, atol=2e-6)
  finally:
    eng.close()


# ---- 7. purity

@pytest.mark.parametrize('name', ['fully_connected', 'pbdg'])
def test_overlap_is_a_pure_measurement(name):
  (plain, _), (meas, _) = _engine(name), _engine(name)
  try:
    for eng in (plain, meas):
      eng.mc_steps(N)
      if eng is meas:
        eng.overlap()
      eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
      if eng is meas:
        eng.overlap(per_chain=True)
    assert _same_words(meas.get_configs(), plain.get_configs())
    assert meas.step_counter == plain.step_counter
    assert _same_words(meas.get_accumulators(), plain.get_accumulators())
    meas.overlap()
    assert _same_words(meas.local_energy()[0], plain.local_energy()[0])
    meas.overlap()
    assert meas.mc_steps(3) == plain.mc_steps(3)
    assert _same_words(meas.get_configs(), plain.get_configs())
    assert meas.step_counter == plain.step_counter
    assert _same_words(meas.amplitude()[0], plain.amplitude()[0])
  finally:
    meas.close(); plain.close()


# ---- 8. refusals

def _refused(eng, error, lam=1.0):
  for call in (lambda: eng.accumulate(MODE2, lam), lambda: eng.epoch_penalized_energy(lam, 1, 1, 1)):
    with pytest.raises(error):
      call()


def _still_usable(eng, fresh):
  assert eng.step_counter == fresh.step_counter and _same_words(eng.get_configs(), fresh.get_configs())
  assert _same_words(eng.local_energy()[0], fresh.local_energy()[0])


def test_refusals_leave_the_engine_usable():
  from tests import test_gpu_buffers as tb
  from tests import test_gpu_renyi as tr
  # a product ctx
  (eng, _), (fresh, _) = _engine(PRODUCT), _engine(PRODUCT)
  try:
    with pytest.raises(NotImplementedError, match='product'):
      eng.overlap()
    _refused(eng, NotImplementedError)
    _still_usable(eng, fresh)
  finally:
    eng.close(); fresh.close()
  # omega unset; a negative, an infinite and a nan lambda; SR reserved
  (eng, _), (fresh, _) = _engine('fully_connected', frozen=False), _engine('fully_connected', frozen=False)
  try:
    with pytest.raises(_hip.HipLibraryError, match='frozen parameters'):
      eng.overlap()
    _refused(eng, _hip.HipLibraryError)
    eng.transfer_params()
    for lam in (-0.5, float('inf'), float('nan')):
      _refused(eng, ValueError, lam)
    eng.sr_reserve(2)
    _refused(eng, _hip.HipLibraryError)
    eng.sr_reserve(0)
    with pytest.raises(ValueError):
      eng.get_gradient(3)
    _still_usable(eng, fresh)
    eng.reset_accumulators(); eng.accumulate(MODE2, 1.0)          # ... and now it runs
    assert eng.get_accumulators()[-2] == 1.0
  finally:
    eng.close(); fresh.close()
  # an output activation other than exp on an unsigned type
  made = []
  try:
    for _ in range(2):
      eng = tr._engine('fully_connected', b=B, output_activation='sigmoid')
      made.append(eng)
      eng.set_params(tr._family('fully_connected')[0]); eng.set_configs(tr._cfg(2, b=B)); eng.set_bonds(tb.TORUS, 1.0, 1.0)
    made[0].transfer_params()
    with pytest.raises(NotImplementedError, match='exp output'):
      made[0].overlap()
    _refused(made[0], NotImplementedError)
    _still_usable(made[0], made[1])
  finally:
    for eng in made:
      eng.close()


# ---- 9. the fused epoch against the same ops one by one

def test_fused_epoch_is_the_ops_one_by_one():
  (fused, _), (byop, _) = _engine('fully_connected'), _engine('fully_connected')
  try:
    fused.epoch_penalized_energy(LAM, N, 3, N, 1e10)
    byop.mc_steps(N, want_accepted=False)
    byop.update_norm(1e10)
    byop.reset_accumulators()
    for _ in range(3):
      byop.accumulate(MODE2, LAM)
      byop.mc_steps(N, want_accepted=False)
    assert _same_words(fused.get_accumulators(), byop.get_accumulators())
    assert _same_words(fused.get_configs(), byop.get_configs())
    assert fused.step_counter == byop.step_counter and fused.get_shift() == byop.get_shift()
    tail = fused.get_accumulators()[-8:]
    assert tail[4] == 3 and tail[6] == 3 and 0 < tail[5] <= 3
  finally:
    fused.close(); byop.close()


# ---- 10. physics, end to end: the first excited state of the 8-site chain

CHAIN = 8
# batch size, learning rate and epochs: DESIGN.md section 4 has the runs behind them (100 epochs of 512 chains passed three
# runs too, but fail one run in five of a numpy model of the update; 256 chains failed one run in three)
TRAIN_HPARAMS = ('batch_size=512,num_batches_per_epoch=1,num_equilibration_sweeps=2,num_monte_carlo_sweeps=1,'
                 'learning_rates=[0.02,0.02,0.02,0.02],top_lin_table_file=top_lin_table.txt,'
                 'bot_lin_table_file=bot_lin_table.txt,ed_vector_file=ed_vector.txt')
TRAIN_EPOCHS = 150


def _fresh_graph():
  from cgs_vmc_amd import session as session_lib, wavefunctions
  session_lib.reset_default_graph()
  wavefunctions.reset_name_scope()


def test_penalised_training_finds_the_first_excited_state(tmp_path, capsys):
  from cgs_vmc_amd import lattice, run_energy_evaluation, run_excited_state_training as rx, run_overlap_evaluation as ro
  from tests import moments_oracle as mo
  mev = _load('make_ed_vector', os.path.join(os.path.dirname(_HERE), 'tools', 'make_ed_vector.py'))
  levels = np.unique(np.round(np.linalg.eigvalsh(mo.dense_h(CHAIN, lattice.chain_bonds(CHAIN), 1.0, 1.0)[1]), 9))
  e0, e1, e2 = levels[:3]
  ground, excited = str(tmp_path / 'ground'), str(tmp_path / 'excited')
  assert abs(mev.main([ground, '--lattice', 'chain', '--size', str(CHAIN)]) - e0) < 1e-8
  mev.main([excited, '--lattice', 'chain', '--size', str(CHAIN)])
  vec = np.loadtxt(os.path.join(ground, 'ed_vector.txt'))
  noise = np.random.default_rng(0).standard_normal(vec.size)
  start = vec + 0.1 * np.linalg.norm(vec) * noise / np.linalg.norm(noise)
  assert (vec @ start) ** 2 / ((vec @ vec) * (start @ start)) >= 0.9
  np.savetxt(os.path.join(excited, 'ed_vector.txt'), start.astype(np.float32), fmt='%.9g')
  for stale in ('checkpoint', 'model_prior_0_epochs.npz'):
    os.remove(os.path.join(excited, stale))
  _fresh_graph()
  rx.main(['--checkpoint_dir', excited, '--lower_state_dir', ground, '--overlap_penalty', '%.17g' % (2 * (e1 - e0)),
           '--num_sites', str(CHAIN), '--wavefunction_type', 'ed_vector', '--heisenberg_jx', '1.0',
           '--num_epochs', str(TRAIN_EPOCHS), '--hparams', TRAIN_HPARAMS])
  fidelities = rx.read_overlap_metrics(excited)
  assert len(fidelities) == TRAIN_EPOCHS and fidelities[0] >= 0.8 and all(0 <= f <= 1 + 1e-6 for f in fidelities)
  with open(os.path.join(excited, 'metrics.txt')) as f:
    assert len(f.read().split()) == TRAIN_EPOCHS
  _fresh_graph()
  result, written = ro.main(['--checkpoint_dir', excited, '--other_dir', ground,
                             '--hparams', 'num_evaluation_samples=20,num_equilibration_sweeps=10'])
  assert [os.path.basename(p) for p in written] == ['overlap.txt']
  assert ro.read_overlap(excited)['fidelity'] == result['fidelity']
  _fresh_graph()
  energy, _ = run_energy_evaluation.main(['--checkpoint_dir', excited, '--heisenberg_jx', '1.0',
                                          '--hparams', 'num_evaluation_samples=20,num_equilibration_sweeps=10'])
  with capsys.disabled():
    print('\nexcited state of the %d-site chain: energy %.6f (E0 %.6f, E1 %.6f, E2 %.6f), fidelity with the ground state '
          '%.3g +/- %.2g, last training estimate %.3g' % (CHAIN, energy, e0, e1, e2, result['fidelity'],
                                                          result['fidelity_err'], fidelities[-1]))
  assert 0.5 * (e0 + e1) < energy < 0.5 * (e1 + e2)
  assert result['fidelity'] <= 0.1

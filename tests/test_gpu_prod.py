"""GPU: the product ctx (vmc_create_product, csrc/vmc_api_prod.hip + prod.hip) against the fp64 product oracle.

Tolerances: the log-amplitudes of the two factors add, so every quantity is held to the SUM of the tolerances the
factors' own tests apply to it (tests/test_gpu_engine.py for fully_connected / rbm, tests/test_gpu_pbdg.py for pbdg,
tests/test_gpu_edvec.py for ed_vector):
  logits     dense 1e-4 absolute (32 units, O(1) values: 32 eps32 |x| ~ 2e-5), pbdg 64 n eps32 kappa(M), ed_vector the fp32
             rounding of ln|v| (4 eps32 |ln|v|| + eps32)
  E_loc      dense 2e-4 max(1, max|ref|); pbdg rtol 2e-3 with atol 2e-3 mean|ref|; ed_vector (n_b + 3) 2^-24
             (|diag| + sum|terms|) of the vector's own terms
  gradients  g1 / g2 sums 2e-3 max|ref| + 1e-4 per factor, the final gradient 2e-3 max|ref| + 2e-4 per factor; scalar
             slots 2e-4 (dense) + 2e-3 (pbdg) relative
  accept     masks equal outside BASELINE.md's band |psi'/psi - sqrt(u)| < 1e-4 psi'/psi
"""
import os

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo
from tests import pbdg_oracle as po
from tests import prod_oracle as pro

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)
N, H = 16, 32
BONDS = vo.torus_bonds(4, 4)
JX, JZ = 1.0, 1.0


def _engine(children, b, **kw):
  from cgs_vmc_amd.engine import VmcEngine
  kw.setdefault('seed', 2024)
  return VmcEngine(N, b, 0, 0, ansatz='prod', children=children, **kw)


def _fc_spec(L):
  return dict(ansatz='fully_connected', num_layers=L, layer_size=H, nonlinearity='relu', output_activation='exp')


RBM_SPEC = dict(ansatz='rbm', num_layers=1, layer_size=H, nonlinearity='relu', output_activation='exp')
PBDG_SPEC = dict(ansatz='pbdg', num_layers=1, layer_size=1)


def _pbdg_theta(seed):
  lim = np.sqrt(3.0 / N)
  return np.random.default_rng(seed).uniform(-lim, lim, N * N).astype(np.float32)


def _pair(name, seed=0):
  """(children specs, oracle Product, per-row logit tolerance fn, signed?)"""
  # (PAIR_TOL below: the factors' own E_loc / accumulator tolerances, summed per pair)
  rng = np.random.default_rng(seed)
  if name == 'pbdg_fc':
    ta, tb = _pbdg_theta(seed + 1), vo.init_params(N, H, 2, rng)
    prod = pro.Product(pro.pbdg_factor(ta), pro.fc_factor(tb, H, 2))
    tol = lambda cfg: 64 * (N // 2) * EPS32 * po.condition_numbers(ta, cfg) + 1e-4
    return [PBDG_SPEC, _fc_spec(2)], prod, tol, True
  if name == 'fc_rbm':
    ta, tb = vo.init_params(N, H, 1, rng), vo.rbm_init_params(N, H, 1, rng)
    prod = pro.Product(pro.fc_factor(ta, H, 1), pro.rbm_factor(tb, H, 1))
    return [_fc_spec(1), RBM_SPEC], prod, lambda cfg: np.full(len(cfg), 2e-4), False
  top, bot, length = eo.lin_tables(N)
  vec = rng.standard_normal(length).astype(np.float32)
  tb = vo.init_params(N, H, 1, rng)
  prod = pro.Product(pro.edvec_factor(vec, top, bot), pro.fc_factor(tb, H, 1))
  spec = dict(ansatz='ed_vector', num_layers=1, layer_size=length, lin_tables=(top, bot))
  tol = lambda cfg: 4 * EPS32 * np.abs(np.log(np.abs(vec[eo.index(cfg, top, bot)]).astype(np.float64))) + EPS32 + 1e-4
  return [spec, _fc_spec(1)], prod, tol, True


def _make(name, b, seed=0, **kw):
  specs, prod, tol, signed = _pair(name, seed)
  eng = _engine(specs, b, **kw)
  assert eng.kernel_path() == 10 and eng.num_params == prod.num_params
  eng.set_params(prod.theta.astype(np.float32))
  np.testing.assert_array_equal(eng.get_params(), prod.theta.astype(np.float32))
  np.testing.assert_array_equal(eng.children[0].get_params(), prod.a.theta.astype(np.float32))
  np.testing.assert_array_equal(eng.children[1].get_params(), prod.b.theta.astype(np.float32))
  eng.set_bonds(BONDS, JX, JZ)
  return eng, prod, tol


# the factors' own tolerances, summed (the log-amplitudes add).  dense (tests/test_gpu_engine.py): E_loc 2e-4 max(1, max|ref|),
# scalar slots 2e-4 relative; pbdg (tests/test_gpu_pbdg.py): E_loc rtol 2e-3 with atol 2e-3 mean|ref|, scalar slots 2e-3
# relative; ed_vector (tests/test_gpu_edvec.py's _eloc_bound): (n_b + 3) 2^-24 (|diag| + sum|terms|) per row, from the
# vector's own diagonal and row terms (n_b of them nonzero).  (dense factors, pbdg factors, ed_vector factors)
PAIR_TOL = {'pbdg_fc': (1, 1, 0), 'edvec_fc': (1, 0, 1), 'fc_rbm': (2, 0, 0)}


def _edvec_eloc_bound(vec, cfg, jx, jz):
  top, bot, _ = eo.lin_tables(N)
  diag, terms = eo.local_energy_terms(vec, cfg, top, bot, BONDS, jx, jz)
  return ((terms != 0).sum(1) + 3) * 2.0 ** -24 * (np.abs(diag) + np.abs(terms).sum(1))


def _eloc_close(e, ref, what, prod, cfg, jx, jz):
  ref = np.asarray(ref, np.float64)
  n_dense, n_pbdg, n_ed = PAIR_TOL[what]
  bound = n_pbdg * (2e-3 * np.abs(ref) + 2e-3 * np.abs(ref).mean()) + n_dense * 2e-4 * max(1.0, np.abs(ref).max())
  if n_ed:
    bound = bound + _edvec_eloc_bound(prod.a.theta, cfg, jx, jz)
  err = np.abs(e - ref)
  k = (err / bound).argmax()
  print('%s E_loc max error %.3g, worst error / bound %.3f (error %.3g, bound %.3g)' % (what, err.max(), err[k] / bound[k], err[k], bound[k]))
  assert (err <= bound).all(), (err[k], bound[k])


@pytest.mark.parametrize('name,b', [('pbdg_fc', 64), ('fc_rbm', 40), ('edvec_fc', 64)])
def test_amplitudes_and_local_energies_match_the_oracle(name, b):
  eng, prod, tol = _make(name, b)
  cfg = vo.random_configurations(N, b, np.random.RandomState(3))
  eng.set_configs(cfg)
  assert eng.get_shift() == 0.0
  with pytest.raises(ValueError):
    eng.set_shift(1.0)
  eng.update_norm()
  sh = [c.get_shift() for c in eng.children]
  logit, psi = eng.amplitude(cfg)
  ref = prod.psi(cfg)
  ref_l = np.log(np.abs(ref))
  err = np.abs(logit.astype(np.float64) - ref_l)
  bound = tol(cfg)
  print('%s logit max error %.3g' % (name, err.max()))
  assert (err <= bound).all(), (err.max(), bound[err.argmax()])
  sure = bound < 0.5
  np.testing.assert_array_equal(np.sign(psi)[sure], np.sign(ref)[sure])
  np.testing.assert_allclose(np.abs(psi), np.exp(logit.astype(np.float64)), rtol=1e-5, atol=1e-37)
  lc, pc = eng.amplitude()                                # the chains' cache: the same kernels, bit for bit
  np.testing.assert_array_equal(lc, logit); np.testing.assert_array_equal(pc, psi)
  assert [c.get_shift() for c in eng.children] == sh
  e, mean = eng.local_energy()
  _eloc_close(e, prod.local_energy(cfg, BONDS, JX, JZ), name, prod, cfg, JX, JZ)
  d, o = eng.local_energy_terms()
  np.testing.assert_allclose(d + o, e, rtol=1e-6, atol=1e-6)
  assert eng.last_connected_rows() == int((cfg[:, [i for i, _ in BONDS]] != cfg[:, [j for _, j in BONDS]]).sum())
  # per-bond couplings, one exchange coupling zero and one negative: the coupling of each row is looked up by its bond
  # and taken once (a wrong bond decode or a coupling taken twice shows here, not at uniform j = 1)
  rng = np.random.default_rng(12)
  jx = rng.uniform(0.3, 1.7, len(BONDS)).astype(np.float32); jx[3] = 0.0; jx[7] = -0.8
  jz = rng.uniform(-1.0, 1.5, len(BONDS)).astype(np.float32)
  eng.set_bonds(BONDS, jx, jz)
  e, _ = eng.local_energy()
  _eloc_close(e, prod.local_energy(cfg, BONDS, jx, jz), name, prod, cfg, jx, jz)
  eng.close()


def test_zero_factors_give_zero_amplitudes_and_finite_neighbour_terms():
  rng = np.random.default_rng(7)
  # a singular pbdg row: two equal rows of the pairing matrix
  ta = _pbdg_theta(3).reshape(N, N); ta[1] = ta[0]
  tb = vo.init_params(N, H, 1, rng)
  eng = _engine([PBDG_SPEC, _fc_spec(1)], 64)
  eng.set_params(np.concatenate([ta.ravel(), tb]))
  cfg = vo.random_configurations(N, 64, np.random.RandomState(4))
  logit, psi = eng.amplitude(cfg)
  both = (cfg[:, 0] > 0) & (cfg[:, 1] > 0)
  assert both.any() and (~both).any()
  assert (psi[both] == 0).all() and np.isneginf(logit[both]).all() and np.isfinite(psi).all() and np.isfinite(logit[~both]).all()
  eng.set_configs(cfg); eng.set_bonds(BONDS, JX, JZ)
  e, _ = eng.local_energy()
  assert np.isfinite(e[~both]).all()                      # singular neighbours add 0
  eng.close()
  # a zero ed_vector entry
  top, bot, length = eo.lin_tables(N)
  vec = rng.standard_normal(length).astype(np.float32)
  idx = eo.index(cfg, top, bot)
  vec[idx[0]] = 0.0
  eng = _engine([dict(ansatz='ed_vector', num_layers=1, layer_size=length, lin_tables=(top, bot)), _fc_spec(1)], 64)
  eng.set_params(np.concatenate([vec, tb]))
  logit, psi = eng.amplitude(cfg)
  zero = idx == idx[0]
  assert (psi[zero] == 0).all() and np.isneginf(logit[zero]).all() and np.isfinite(psi).all()
  eng.set_configs(cfg); eng.set_bonds(BONDS, JX, JZ)
  e, _ = eng.local_energy()
  assert np.isfinite(e[~zero]).all()
  eng.close()


def test_sampler_injected_steps_cache_proposals_and_reruns(monkeypatch):
  from cgs_vmc_amd import graph_builders
  from cgs_vmc_amd.engine import VmcEngine
  b = 64
  eng, prod, _ = _make('pbdg_fc', b)
  cfg = vo.random_configurations(N, b, np.random.RandomState(5))
  eng.set_configs(cfg)
  rng = np.random.default_rng(6)
  cur = cfg.copy()
  n_band = 0
  for step in range(200):
    i_up = np.array([rng.choice(np.flatnonzero(r > 0)) for r in cur], np.int32)
    i_dn = np.array([rng.choice(np.flatnonzero(r < 0)) for r in cur], np.int32)
    u = rng.random(b).astype(np.float32)
    mask = eng.mc_step_injected(i_up, i_dn, u)
    new, acc, ratio = pro.mc_step(prod, cur, i_up, i_dn, u)
    band = np.abs(np.abs(ratio) - np.sqrt(u.astype(np.float64))) < 1e-4 * np.abs(ratio)
    n_band += int(band.sum())
    assert (mask[~band] == acc[~band]).all(), step
    rows = np.arange(b)
    nxt = cur.copy()
    nxt[rows[mask], i_up[mask]] = -1.0
    nxt[rows[mask], i_dn[mask]] = 1.0
    cur = nxt
    if step % 50 == 49:
      np.testing.assert_array_equal(eng.get_configs(), cur)       # the chains are exactly the accepted exchanges
  assert n_band < 20
  lc, pc = eng.amplitude()
  lr, pr = eng.amplitude(cur)
  np.testing.assert_array_equal(lc, lr); np.testing.assert_array_equal(pc, pr)
  # the proposals every sampler draws: a plain fully_connected ctx with the same seed, step and chains
  plain = VmcEngine(N, b, 1, H, seed=2024)
  plain.set_params(vo.init_params(N, H, 1, np.random.default_rng(0)))
  plain.set_configs(cur)
  for step in (0, 7, 2 ** 33 + 1):
    for x, y in zip(eng.debug_proposals(step), plain.debug_proposals(step)):
      np.testing.assert_array_equal(x, y)
  # mc_steps(n) replayed: the proposals k_prod_accept draws for steps 1 .. n-1 (its own copy of the rule, from the spins
  # as patched after the commit) must be the ones k_wide_propose draws on a plain ctx for the chains as they then stand
  # -- with the oracle's verdicts, the replay ends in the sampler's chains unless a verdict fell into the band
  start, step0, n_rep = cur.copy(), eng.step_counter, 12
  accepted = eng.mc_steps(n_rep)
  assert eng.step_counter == step0 + n_rep
  rep, n_acc, banded = start.copy(), 0, np.zeros(b, bool)
  for k in range(n_rep):
    plain.set_configs(rep)
    i_up, i_dn, u = plain.debug_proposals(step0 + k)
    rep, acc, ratio = pro.mc_step(prod, rep, i_up, i_dn, u)
    banded |= np.abs(np.abs(ratio) - np.sqrt(u.astype(np.float64))) < 1e-4 * np.abs(ratio)
    n_acc += int(acc.sum())
  assert banded.sum() <= 2
  np.testing.assert_array_equal(eng.get_configs()[~banded], rep[~banded])
  assert banded.any() or accepted == n_acc
  plain.close()
  eng.close()
  monkeypatch.setenv('CGS_VMC_SEED', '77')
  assert graph_builders.sampler_seed() == 77
  runs = []
  for _ in range(2):
    e2, _, _ = _make('pbdg_fc', 40, seed=graph_builders.sampler_seed())
    e2.set_configs(cfg[:40])
    accepted = e2.mc_steps(3 * N)
    lc, _ = e2.amplitude(); lr, _ = e2.amplitude(e2.get_configs())
    np.testing.assert_array_equal(lc, lr)
    assert e2.step_counter == 3 * N and 0 < accepted < 40 * 3 * N
    runs.append((e2.get_configs(), accepted))
    e2.close()
  np.testing.assert_array_equal(runs[0][0], runs[1][0])
  assert runs[0][1] == runs[1][1] and (runs[0][0].sum(1) == 0).all()


@pytest.mark.parametrize('name,b', [('pbdg_fc', 64), ('fc_rbm', 40)])
def test_accumulators_of_both_modes_match_the_oracle(name, b):
  eng, prod, _ = _make(name, b)
  cfg = vo.random_configurations(N, b, np.random.RandomState(8))
  eng.set_configs(cfg)
  pa, p = prod.a.num_params, prod.num_params
  # EnergyGradient
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  acc = vo.Accumulators(p, np.float64)
  pro.energy_gradient_accumulate(acc, prod, cfg, BONDS, JX, JZ)
  res = eng.get_accumulators()

  def close(got, ref, what, atol=2e-4):                     # g1 / g2: 2e-3 max + 1e-4 per factor; the gradients: + 2e-4 per factor
    err = np.abs(got - ref).max()
    bound = 4e-3 * np.abs(ref).max() + atol
    print('%s %s max error %.3g (bound %.3g)' % (name, what, err, bound))
    assert err <= bound, (what, err, bound)
  close(res[:pa], acc.g1_total[:pa], 'g1_a'); close(res[pa:p], acc.g1_total[pa:], 'g1_b')
  close(res[p:p + pa], acc.g2_total[:pa], 'g2_a'); close(res[p + pa:2 * p], acc.g2_total[pa:], 'g2_b')
  sc_tol = PAIR_TOL[name][0] * 2e-4 + PAIR_TOL[name][1] * 2e-3    # (no ed_vector pair here)
  print('%s e_total error %.3g (bound %.3g)' % (name, abs(res[2 * p] - acc.e_total), sc_tol * max(1, abs(acc.e_total))))
  assert abs(res[2 * p] - acc.e_total) < sc_tol * max(1, abs(acc.e_total)) and res[2 * p + 1] == b and res[2 * p + 4] == 1
  close(eng.get_gradient(_hip.VMC_MODE_ENERGY_GRADIENT), vo.energy_gradient(acc), 'gradient', 4e-4)
  # LogOverlapITSWO with a perturbed supervisor: ratios of both signs where a factor is signed
  rng = np.random.default_rng(9)
  tw = (prod.theta + 0.3 * rng.standard_normal(p) * np.abs(prod.theta).mean()).astype(np.float32)
  eng.set_params(tw, _hip.VMC_OMEGA)
  specs, _, _, signed = _pair(name)
  fa = pro.pbdg_factor(tw[:pa]) if name == 'pbdg_fc' else pro.fc_factor(tw[:pa], H, 1)
  fb = pro.fc_factor(tw[pa:], H, 2) if name == 'pbdg_fc' else pro.rbm_factor(tw[pa:], H, 1)
  omega = pro.Product(fa, fb)
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.05)
  acc = vo.Accumulators(p, np.float64)
  _, ratio = pro.log_overlap_accumulate(acc, prod, omega, cfg, BONDS, JX, JZ, 0.05)
  if signed:
    assert (ratio > 0).any() and (ratio < 0).any()
  res = eng.get_accumulators()
  close(res[:p], acc.g1_total, 'itswo g1'); close(res[p:2 * p], acc.g2_total, 'itswo g2')
  print('%s itswo e_total error %.3g (bound %.3g), r_total error %.3g (bound %.3g)' % (
      name, abs(res[2 * p] - acc.e_total), sc_tol * max(1, abs(acc.e_total)), abs(res[2 * p + 2] - acc.r_total),
      sc_tol * max(1, np.abs(ratio).sum())))
  assert abs(res[2 * p] - acc.e_total) < sc_tol * max(1, abs(acc.e_total))
  assert abs(res[2 * p + 2] - acc.r_total) < sc_tol * max(1, np.abs(ratio).sum())
  close(eng.get_gradient(_hip.VMC_MODE_LOG_OVERLAP_ITSWO), vo.log_overlap_gradient(acc), 'itswo gradient', 4e-4)
  eng.close()


def test_epoch_entries_equal_the_op_sequence_bit_for_bit():
  b, n_eq, nb, n_mc = 40, 8, 2, 4
  cfg = vo.random_configurations(N, b, np.random.RandomState(10))
  out = []
  for fused in (True, False):
    eng, prod, _ = _make('pbdg_fc', b)
    eng.set_configs(cfg)
    if fused:
      eng.epoch_energy_gradient(n_eq, nb, n_mc, 1e10)
    else:
      eng.mc_steps(n_eq); eng.update_norm(1e10); eng.reset_accumulators()
      for _ in range(nb):
        eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT); eng.mc_steps(n_mc)
    e1 = eng.apply_adam(_hip.VMC_MODE_ENERGY_GRADIENT, 1e-2)
    th1 = eng.get_params()
    if fused:
      e2 = eng.epoch_log_overlap(0.05, n_eq, nb, n_mc, 1e10, 1e-2, 0.9, 0.99, 1e-8)
    else:
      eng.mc_steps(n_eq); eng.update_norm(1e10); eng.transfer_params()
      for _ in range(nb):
        eng.mc_steps(n_mc); eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.05)
        eng.apply_adam(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 1e-2, 0.9, 0.99, 1e-8)
      e2 = eng.mean_energy()
    th2 = eng.get_params()
    assert np.isfinite(th2).all() and not np.array_equal(th1, prod.theta.astype(np.float32)) and not np.array_equal(th1, th2)
    if fused:
      means, accepted = eng.evaluate(None, n_eq, 3, n_mc)
    else:
      eng.mc_steps(n_eq)
      means, accepted = [], 0
      for _ in range(3):
        means.append(eng.local_energy(want_eloc=False)[1]); accepted += eng.mc_steps(n_mc)
    out.append((e1, th1, e2, th2, np.asarray(means), accepted, eng.get_configs(), eng.get_adam_state()))
    eng.close()
  for x, y in zip(out[0], out[1]):
    if isinstance(x, tuple):
      for xx, yy in zip(x, y):
        np.testing.assert_array_equal(xx, yy)
    else:
      np.testing.assert_array_equal(x, y)


def test_refusals_and_life_cycle():
  import ctypes as C
  from cgs_vmc_amd.engine import VmcEngine
  lib = _hip.load()
  a = VmcEngine(N, 64, 1, 1, ansatz='pbdg')
  bad_b = VmcEngine(N, 40, 1, H)
  out = C.c_void_p()
  assert lib.vmc_create_product(a._ctx, bad_b._ctx, C.byref(out)) == _hip.VMC_ERR_INVALID and not out.value
  tanh = VmcEngine(N, 64, 1, H, output_activation='tanh')
  assert lib.vmc_create_product(a._ctx, tanh._ctx, C.byref(out)) == _hip.VMC_ERR_UNSUPPORTED
  conv = VmcEngine(N, 64, 2, 8, ansatz='conv_2d', kernel_size=3, size_x=4, size_y=4)
  assert lib.vmc_create_product(a._ctx, conv._ctx, C.byref(out)) == _hip.VMC_ERR_UNSUPPORTED
  for e in (bad_b, tanh, conv, a):
    e.close()
  with pytest.raises(NotImplementedError):
    _engine([PBDG_SPEC, dict(_fc_spec(1), output_activation='tanh')], 64)
  with pytest.raises(ValueError):
    VmcEngine(N, 64, 1, 1, ansatz='prod')
  desc = _hip.VmcDesc(N, 64, 1, H, 0, 1, 0, 0, _hip.ANSATZ_PRODUCT, 0, 1, None, 0, 0, 0, 0)
  assert lib.vmc_create(C.byref(desc), C.byref(out)) == _hip.VMC_ERR_INVALID
  for _ in range(3):                                       # create / destroy is clean, three times
    eng, prod, _ = _make('pbdg_fc', 64)
    cfg = vo.random_configurations(N, 64, np.random.RandomState(11))
    eng.set_configs(cfg)
    ca, cb = eng.children
    # a factor while composed: chain-state entries refuse, parameter / shift / host-row entries work
    for call in (lambda: ca.set_configs(cfg), lambda: ca.mc_steps(1), lambda: cb.accumulate(0),
                 lambda: cb.epoch_energy_gradient(1, 1, 1), lambda: cb.local_energy(), lambda: cb.amplitude()):
      with pytest.raises(ValueError, match='error -4') as info:      # VMC_ERR_STATE, a ValueError in Python
        call()
      assert isinstance(info.value, _hip.HipLibraryError)
    la, _ = ca.amplitude(cfg); lb, _ = cb.amplitude(cfg)
    lp, _ = eng.amplitude(cfg)
    np.testing.assert_allclose(lp, (la - ca.get_shift()) + (lb - cb.get_shift()), rtol=0, atol=0)
    cb.set_shift(-3.0)
    assert eng.amplitude(cfg)[0][0] == (la[0] - ca.get_shift()) + (lb[0] + 3.0)
    # a product of products
    other = VmcEngine(N, 64, 1, H)
    assert lib.vmc_create_product(eng._ctx, other._ctx, C.byref(out)) == _hip.VMC_ERR_UNSUPPORTED
    assert lib.vmc_create_product(ca._ctx, other._ctx, C.byref(out)) == _hip.VMC_ERR_STATE
    other.close()
    with pytest.raises(NotImplementedError, match='prod'):
      eng.sr_reserve(2)
    with pytest.raises(NotImplementedError, match='prod'):
      eng.sr_solve(0.01, 1e-3, 10)
    with pytest.raises(NotImplementedError, match='prod'):
      eng.sweep_tile()
    means = np.empty(1)
    assert lib.vmc_evaluate(eng._ctx, None, 2, 0, 1, 1, means.ctypes.data_as(C.POINTER(C.c_double)), None) == _hip.VMC_ERR_UNSUPPORTED
    assert lib.vmc_allreduce_accumulators(eng._ctx, None, 2) == _hip.VMC_ERR_UNSUPPORTED
    assert lib.vmc_epoch_energy_gradient_dist(eng._ctx, None, 2, 1, 1, 1, C.c_float(0)) == _hip.VMC_ERR_UNSUPPORTED
    # destroying the product frees the factors: they work alone again
    ctx, eng._ctx = eng._ctx, C.c_void_p()
    lib.vmc_destroy(ctx)
    ca.set_configs(cfg); ca.set_bonds(BONDS, JX, JZ)
    assert ca.mc_steps(4) >= 0 and np.isfinite(ca.local_energy()[1])
    eng.close()
    assert not ca._ctx.value and not cb._ctx.value


def _ed_spec(length, top, bot):
  return dict(ansatz='ed_vector', num_layers=1, layer_size=length, lin_tables=(top, bot))


def test_exact_ground_state_factorised_has_the_exact_local_energy():
  """4 x 4 torus, jx = +1, exact ground state v (both signs): ed_vector(sign(v) sqrt|v|) x ed_vector(sqrt|v|) = v has
  E_loc = E0 = -11.22848 on every sampled configuration (|v| >= 1e-5 everywhere on the torus).  Bound: the absolute
  bound tests/test_gpu_edvec.py applies to the single vector, (n_b + 3) 2^-24 (|diag| + sum|terms|), doubled.  Then
  ed_vector(v) x fully_connected with all weights zero: the same E_loc, and the accept masks of ed_vector(v) alone."""
  from cgs_vmc_amd.engine import VmcEngine
  e0, vec64, top, bot = eo.vector_from_ed(N, BONDS, 1.0, 1.0)
  assert abs(e0 + 11.22848) < 1e-5 and (vec64 > 0).any() and (vec64 < 0).any()
  length = len(vec64)
  u = (np.sign(vec64) * np.sqrt(np.abs(vec64))).astype(np.float32)
  w = np.sqrt(np.abs(vec64)).astype(np.float32)
  b = 1024
  cfg = vo.random_configurations(N, b, np.random.RandomState(13))
  assert (np.abs(vec64[eo.index(cfg, top, bot)]) >= 1e-5).all()

  def bound_of(vec):
    diag, terms = eo.local_energy_terms(vec, cfg, top, bot, BONDS, 1.0, 1.0)
    return 2 * ((terms != 0).sum(1) + 3) * 2.0 ** -24 * (np.abs(diag) + np.abs(terms).sum(1))
  eng = _engine([_ed_spec(length, top, bot), _ed_spec(length, top, bot)], b)
  eng.set_params(np.concatenate([u, w])); eng.set_bonds(BONDS, 1.0, 1.0); eng.set_configs(cfg)
  logit, psi = eng.amplitude()
  ref = u.astype(np.float64)[eo.index(cfg, top, bot)] * w.astype(np.float64)[eo.index(cfg, top, bot)]
  np.testing.assert_array_equal(np.sign(psi), np.sign(ref))
  np.testing.assert_allclose(psi, ref, rtol=1e-5)
  e = eng.local_energy()[0].astype(np.float64)
  bound = bound_of(u.astype(np.float64) * w.astype(np.float64))
  worst = (np.abs(e - e0) / bound).max()
  print('exact pin u x w: max |E_loc - E0| = %.3g, worst error / bound = %.3f' % (np.abs(e - e0).max(), worst))
  assert worst <= 1.0, worst
  eng.close()
  # ed_vector(v) x a fully_connected factor with all weights zero (a constant): E_loc and the sampler of the vector alone
  v32 = vec64.astype(np.float32)
  zero = np.zeros(vo.num_params(N, H, 1), np.float32)
  eng = _engine([_ed_spec(length, top, bot), _fc_spec(1)], b)
  eng.set_params(np.concatenate([v32, zero])); eng.set_bonds(BONDS, 1.0, 1.0); eng.set_configs(cfg)
  alone = VmcEngine(N, b, 1, length, ansatz='ed_vector', lin_tables=(top, bot), seed=2024)
  alone.set_params(v32); alone.set_bonds(BONDS, 1.0, 1.0); alone.set_configs(cfg)
  e = eng.local_energy()[0].astype(np.float64)
  worst = (np.abs(e - e0) / bound_of(v32.astype(np.float64))).max()
  print('exact pin v x 1: max |E_loc - E0| = %.3g, worst error / bound = %.3f' % (np.abs(e - e0).max(), worst))
  assert worst <= 1.0, worst
  rng = np.random.default_rng(14)
  cur = cfg.copy()
  for step in range(6):
    i_up = np.array([rng.choice(np.flatnonzero(r > 0)) for r in cur], np.int32)
    i_dn = np.array([rng.choice(np.flatnonzero(r < 0)) for r in cur], np.int32)
    uu = rng.random(b).astype(np.float32)
    new = cur.copy(); rows = np.arange(b); new[rows, i_up] = -1.0; new[rows, i_dn] = 1.0
    ratio = np.abs(vec64[eo.index(new, top, bot)] / vec64[eo.index(cur, top, bot)])
    band = np.abs(ratio - np.sqrt(uu.astype(np.float64))) < 1e-4 * ratio
    m_prod, m_alone = eng.mc_step_injected(i_up, i_dn, uu), alone.mc_step_injected(i_up, i_dn, uu)
    assert band.sum() <= 3 and (m_prod[~band] == m_alone[~band]).all() and m_alone.any()
    if (m_prod != m_alone).any():
      break                                               # (a verdict inside the band: the chains differ from here on)
    cur = np.where(m_alone[:, None], new, cur)
    np.testing.assert_array_equal(eng.get_configs(), alone.get_configs())
  eng.close(); alone.close()


def test_prod_run_training_resume_and_energy_evaluation(tmp_path, monkeypatch):
  """run_training --wavefunction_type=prod (pbdg x fully_connected) on the 4 x 4 torus at jx = +1 (E0 = -11.22848): 30
  EnergyGradient epochs, --resume_training from .npz and from a TF bundle, run_energy_evaluation (E >= E0 within three
  standard errors, E < the Neel state's -8.0), the checkpoint's variable names, ten LogOverlapITSWO epochs, and the
  refusal of StochasticReconfiguration."""
  from cgs_vmc_amd import lattice, run_energy_evaluation, run_training, session, wavefunctions
  e0 = -11.22848
  monkeypatch.setenv('CGS_VMC_INIT_SEED', '7')
  hp = ('batch_size=512,num_equilibration_sweeps=10,num_batches_per_epoch=20,learning_rates=[0.03,0.03],'
        'learning_rate_stops=[1000],num_evaluation_samples=20,num_fc_layers=1,fc_layer_size=32,'
        'composite_wavefunction_types=[pbdg,fully_connected],composite_output_activations=[exp,exp]')
  names = {'projected_bdg/pairing_matrix', 'fully_connected_network/linear/w', 'fully_connected_network/linear/b',
           'fully_connected_network/linear_1/w', 'fully_connected_network/linear_1/b'}

  def fresh():
    session.reset_default_graph(); wavefunctions.reset_name_scope()

  def run(d, opt, epochs, resume=False):
    fresh()
    run_training.main(['--checkpoint_dir', d, '--num_sites', '16', '--heisenberg_jx', '1.0', '--wavefunction_type', 'prod',
                       '--optimizer', opt, '--num_epochs', str(epochs), '--hparams', hp] +
                      (['--resume_training', 'true'] if resume else []))
    return [float(x) for x in open(os.path.join(d, 'metrics.txt')).read().split()]
  for fmt in ('npz', 'tf'):
    monkeypatch.setenv('CGS_VMC_CHECKPOINT_FORMAT', fmt)
    d = str(tmp_path / fmt)
    os.makedirs(d)
    lattice.write_bonds(d, lattice.torus_bonds(4, 4))
    epochs = 30 if fmt == 'npz' else 4
    energies = run(d, 'EnergyGradient', epochs)
    assert len(energies) == epochs and np.isfinite(energies).all() and energies[-1] < energies[0], energies
    resumed = run(d, 'EnergyGradient', 2, resume=True)[epochs:]
    assert len(resumed) == 2 and np.isfinite(resumed).all() and resumed[0] < energies[0], (resumed, energies)
    if fmt == 'tf':
      assert not any(f.endswith('.npz') for f in os.listdir(d))
      continue
    ckpt = session.latest_checkpoint(d)
    assert set(np.load(ckpt + '.npz').files) == names
    fresh()
    samples = run_energy_evaluation.evaluate(run_energy_evaluation.cli_common.parser_from_table(
        '', run_energy_evaluation.FLAG_TABLE).parse_args(['--checkpoint_dir', d, '--heisenberg_jx', '1.0']))
    mean, se = samples.mean(), samples.std(ddof=1) / np.sqrt(len(samples))
    print('prod 4x4 EnergyGradient: first epoch E %.4f, epoch 30 E %.4f, evaluated E %.4f +/- %.4f (exact %.5f)'
          % (energies[0], energies[-1], mean, se, e0))
    assert mean > e0 - 3 * se, (mean, se)
    assert mean < -8.0, (mean, energies[-5:])
    itswo = run(d, 'LogOverlapITSWO', 10, resume=True)[epochs + 2:]
    assert len(itswo) == 10 and np.isfinite(itswo).all(), itswo
  fresh()
  d = str(tmp_path / 'sr')
  os.makedirs(d)
  lattice.write_bonds(d, lattice.torus_bonds(4, 4))
  with pytest.raises(NotImplementedError, match='prod'):
    run_training.main(['--checkpoint_dir', d, '--num_sites', '16', '--heisenberg_jx', '1.0', '--wavefunction_type', 'prod',
                       '--optimizer', 'StochasticReconfiguration', '--num_epochs', '2', '--hparams', hp])
  fresh()

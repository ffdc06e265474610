"""GPU parity of the ed_vector ansatz -- FullVector (wavefunctions.py:1001-1080) on csrc/edvec.hip -- through the C ABI
and the front end, against the fp64 oracle tests/edvec_oracle.py: amplitudes bit for bit, local energies of exact signed
ground states within the rounding bound of the fp32 pipeline, evaluation, the sampler, the gradient scatter with
collisions (bit-identical reruns), sharded chains, training and the ctx life cycle.

Rounding bounds (u = 2^-24).  A local energy is diag (exact: multiples of 1/4) plus n_b terms of one division and one
multiplication each (2 u), summed by a tree of depth <= ceil(log2 n_b) <= n_b and added to diag (1 u): the issue's
(n_b + 3) u (|diag| + sum |terms|).  A gradient entry sums c chains' terms -- one division each in double, the sum in
double -- then rounds once and is added once to the accumulator: within (c + 2) u sum |terms|."""
import os

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _square_bonds(lx, ly):
  return sorted({(min(i, j), max(i, j)) for i, j in vo.torus_bonds(lx, ly) if i != j})


def _engine(n, b, length, tables=None, **kw):
  from cgs_vmc_amd.engine import VmcEngine
  kw.setdefault('seed', 2024)
  return VmcEngine(n, b, 1, length, ansatz='ed_vector', lin_tables=tables, **kw)


def _random_sz0(n, rows, seed):
  rng = np.random.default_rng(seed)
  cfg = -np.ones((rows, n), np.float32)
  for r in cfg:
    r[rng.permutation(n)[:n // 2]] = 1.0
  return cfg


def _check_amplitudes(eng, vec, cfg, top, bot):
  logit, psi = eng.amplitude(cfg)
  want = vec[eo.index(cfg, top, bot)]
  np.testing.assert_array_equal(psi.view(np.uint32), want.view(np.uint32))          # bit for bit
  with np.errstate(divide='ignore'):
    ref = np.log(np.abs(want.astype(np.float64)))
  nz = want != 0
  ulp = np.spacing(np.abs(ref[nz]).astype(np.float32)).astype(np.float64)
  err = np.abs(logit[nz].astype(np.float64) - ref[nz])
  assert (err <= ulp).all(), (err / ulp).max()
  assert np.isneginf(logit[~nz]).all()


def test_edvec_amplitudes_are_the_gathered_entries_bit_for_bit():
  n = 16
  top, bot, length = eo.lin_tables(n)
  vec = np.random.default_rng(1).standard_normal(length).astype(np.float32)
  vec[::97] = 0.0                                                                   # planted zeros
  cfg = eo.sz0_configurations(n)
  eng = _engine(n, 64, length, (top, bot))
  assert eng.kernel_path() == 9 and eng.num_params == length
  eng.set_params(vec)
  _check_amplitudes(eng, vec, cfg, top, bot)
  _, psi = eng.amplitude(cfg)
  assert (psi == 0).sum() == len(range(0, length, 97))
  eng.set_configs(cfg[:64])
  lc, pc = eng.amplitude()
  lr, pr = eng.amplitude(cfg[:64])
  np.testing.assert_array_equal(lc, lr); np.testing.assert_array_equal(pc, pr)
  bad = cfg[:1].copy(); bad[0, np.flatnonzero(bad[0] < 0)[0]] = 1.0
  with pytest.raises(ValueError):
    eng.amplitude(bad)
  with pytest.raises(NotImplementedError):
    eng.sr_reserve(2)
  eng.close()


def test_edvec_amplitudes_n28_past_the_l2():
  import torch
  n = 28
  top, bot, length = eo.lin_tables(n)
  need = 8 * 4 * length + (1 << 30)                 # seven vectors of the ctx and head room
  free = torch.cuda.mem_get_info()[0]
  if free < need:
    print('ed_vector N = 28 amplitudes SKIPPED: %.1f GB of device memory free, %.1f GB needed' % (free / 1e9, need / 1e9))
    pytest.skip('device memory short for the 160 MB vector (7 buffers of it)')
  vec = np.random.default_rng(2).standard_normal(length, dtype=np.float32)
  cfg = _random_sz0(n, 4096, 3)
  eng = _engine(n, 64, length, (top, bot))
  eng.set_params(vec)
  _check_amplitudes(eng, vec, cfg, top, bot)
  eng.close()


def _exact_case(name):
  n = 16
  bonds = _square_bonds(4, 4) if name == 'torus-4x4' else [tuple(b) for b in vo.chain_bonds(16)]
  e0, vec64, top, bot = eo.vector_from_ed(n, bonds, 1.0, 1.0)
  return n, bonds, e0, vec64, top, bot


def _eloc_bound(vec32, cfg, top, bot, bonds):
  diag, terms = eo.local_energy_terms(vec32, cfg, top, bot, bonds, 1.0, 1.0)
  n_b = (terms != 0).sum(1)
  return diag + terms.sum(1), (n_b + 3) * U * (np.abs(diag) + np.abs(terms).sum(1))


@pytest.mark.parametrize('name', ['torus-4x4', 'chain-16'])
def test_edvec_exact_signed_state_has_the_oracles_local_energies(name):
  """jx = +1: the ground state carries both signs.  Measured on an MI355X: worst error / bound 0.111 (torus), 0.231 (chain)."""
  n, bonds, e0, vec64, top, bot = _exact_case(name)
  assert (vec64 > 0).any() and (vec64 < 0).any()
  cfg = eo.sz0_configurations(n)
  # pins the oracle: E_loc = E0 to 1e-9 on the unrounded vector.  eigsh converges the residual r = H v - E0 v to about
  # 1e-15 |H| per component and E_loc - E0 = r_k / v_k, so the figure is asked where |v_k| >= 1e-5 (every configuration
  # of the torus; the chain's ground state has components down to 3e-9) and the residual itself everywhere
  psi64 = vec64[eo.index(cfg, top, bot)]
  nz64 = psi64 != 0
  dev = np.zeros(len(cfg))
  dev[nz64] = eo.local_energy(vec64, cfg[nz64], top, bot, bonds, 1.0, 1.0) - e0
  assert np.abs(dev[np.abs(psi64) >= 1e-5]).max() < 1e-9 and np.abs(dev * psi64).max() < 1e-13
  assert name != 'torus-4x4' or (np.abs(psi64) >= 1e-5).all()
  vec = vec64.astype(np.float32)
  cfg = cfg[vec[eo.index(cfg, top, bot)] != 0]
  ref, bound = _eloc_bound(vec, cfg, top, bot, bonds)
  b = 4096
  eng = _engine(n, b, len(vec), (top, bot))
  eng.set_params(vec); eng.set_bonds(bonds, 1.0, 1.0)
  worst = 0.0
  for r0 in range(0, len(cfg), b):
    rows = cfg[r0:r0 + b]
    pad = np.concatenate([rows, np.repeat(rows[:1], b - len(rows), 0)])
    eng.set_configs(pad)
    eloc = eng.local_energy()[0][:len(rows)].astype(np.float64)
    ratio = np.abs(eloc - ref[r0:r0 + b]) / bound[r0:r0 + b]
    worst = max(worst, ratio.max())
    d, o = eng.local_energy_terms()
    np.testing.assert_array_equal((d + o)[:len(rows)], eloc.astype(np.float32))
  print('ed_vector %s: worst |E_loc - oracle| / bound = %.3f over %d configurations' % (name, worst, len(cfg)))
  assert worst <= 1.0, 'worst error / bound = %.3f' % worst
  eng.close()


def test_edvec_evaluation_of_the_exact_state(tmp_path):
  """vmc_evaluate and the run_energy_evaluation CLI (MonteCarloOperatorEvaluator) on the 4 x 4 ground state: zero variance."""
  n, bonds, e0, vec64, top, bot = _exact_case('torus-4x4')
  vec = vec64.astype(np.float32)
  cfg = eo.sz0_configurations(n)
  cfg = cfg[vec[eo.index(cfg, top, bot)] != 0]
  tol = _eloc_bound(vec, cfg, top, bot, bonds)[1].max()
  # (the fp32-rounded vector is an eigenvector only to 2^-24 per entry: its own E_loc spread is printed beside the bound)
  spread = np.abs(eo.local_energy(vec, cfg, top, bot, bonds, 1.0, 1.0) - e0).max()
  b = 1024
  eng = _engine(n, b, len(vec), (top, bot))
  eng.set_params(vec); eng.set_bonds(bonds, 1.0, 1.0)
  eng.set_configs(vo.random_configurations(n, b, np.random.RandomState(4)))
  means, accepted = eng.evaluate(None, 100, 10, 16)
  print('ed_vector evaluate: max |mean - E0| = %.3g (bound %.3g; E_loc spread of the rounded vector %.3g)' % (np.abs(means - e0).max(), tol, spread))
  assert accepted > 0 and (np.abs(means - e0) <= tol).all(), (means - e0, tol, spread)
  eng.close()
  from cgs_vmc_amd import run_energy_evaluation, session, wavefunctions
  from tools import make_ed_vector as mk
  d = str(tmp_path / 'ed')
  e0_tool = mk.main([d, '--lattice', 'square', '--size', '4', '4'])
  assert abs(e0_tool - e0) < 1e-9
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  mean, _ = run_energy_evaluation.main(['--checkpoint_dir', d, '--heisenberg_jx', '1.0',
                                        '--hparams', 'batch_size=256,num_evaluation_samples=5,num_equilibration_sweeps=5'])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  assert abs(mean - e0) <= tol, (mean, e0, tol)


def _injection(seed, n, b, vec, top, bot):
  """Proposals and the fp64 oracle's verdicts: (cfg, i_up, i_dn, u, accept, near) with near = within 4 ulp (fp32) of the threshold."""
  rng = np.random.default_rng(seed)
  cfg = _random_sz0(n, b, seed + 1)
  i_up = np.array([rng.choice(np.flatnonzero(r > 0)) for r in cfg])
  i_dn = np.array([rng.choice(np.flatnonzero(r < 0)) for r in cfg])
  u = rng.uniform(0, 1, b).astype(np.float32)
  new = cfg.copy()
  new[np.arange(b), i_up] = -1.0; new[np.arange(b), i_dn] = 1.0
  with np.errstate(divide='ignore', invalid='ignore'):
    q2 = (vec[eo.index(new, top, bot)].astype(np.float64) / vec[eo.index(cfg, top, bot)].astype(np.float64)) ** 2
  near = np.abs(q2 - u) <= 4 * np.spacing(u).astype(np.float64)
  return cfg, i_up, i_dn, u, q2 > u, near


def test_edvec_sampler_injected_replayed_cached_and_zero_starts(monkeypatch):
  n, b = 16, 256
  top, bot, length = eo.lin_tables(n)
  vec = np.random.default_rng(5).standard_normal(length).astype(np.float32)
  cfg, i_up, i_dn, u, want, near = _injection(6, n, b, vec, top, bot)
  assert near.sum() <= 0.01 * b                          # (seed 6: none; checked on the CPU)
  eng = _engine(n, b, length, (top, bot))
  eng.set_params(vec); eng.set_configs(cfg)
  mask = eng.mc_step_injected(i_up, i_dn, u)
  np.testing.assert_array_equal(mask[~near], want[~near])
  moved = eng.get_configs()
  new = cfg.copy(); new[np.arange(b), i_up] = -1.0; new[np.arange(b), i_dn] = 1.0
  np.testing.assert_array_equal(moved, np.where(mask[:, None], new, cfg))
  # the proposals are the project's rule; a replay from a saved step counter gives identical chains
  eng.set_configs(cfg)
  eng.step_counter = 7
  pu, pd, pv = eng.debug_proposals(7)
  u_sites, u_acc = vo.step_uniforms(2024, np.arange(b), 7, n)
  iu, idn = vo.propose_exchange(cfg, u_sites)
  np.testing.assert_array_equal(pu, iu); np.testing.assert_array_equal(pd, idn); np.testing.assert_array_equal(pv, u_acc)
  eng.mc_steps(50)
  saved, mid = eng.step_counter, eng.get_configs()
  assert saved == 57
  eng.mc_steps(150)
  first = eng.get_configs()
  assert (first.sum(1) == 0).all()                       # Sz stays 0
  lc, pc = eng.amplitude()                               # the cached psi equals a fresh vmc_amplitude
  lr, pr = eng.amplitude(first)
  np.testing.assert_array_equal(lc.view(np.uint32), lr.view(np.uint32)); np.testing.assert_array_equal(pc.view(np.uint32), pr.view(np.uint32))
  np.testing.assert_array_equal(pr, vec[eo.index(first, top, bot)])
  eng.set_configs(mid)
  eng.step_counter = saved
  eng.mc_steps(150)
  np.testing.assert_array_equal(eng.get_configs(), first)
  eng.close()
  # the same chains with the tables read through L2 instead of LDS
  monkeypatch.setenv('CGS_VMC_EDVEC_TABLES_LDS', '0')
  eng = _engine(n, b, length, (top, bot))
  eng.set_params(vec); eng.set_configs(mid)
  eng.step_counter = saved
  eng.mc_steps(150)
  np.testing.assert_array_equal(eng.get_configs(), first)
  eng.close()
  monkeypatch.delenv('CGS_VMC_EDVEC_TABLES_LDS')
  # a chain on a zero-amplitude configuration leaves it at the first non-zero proposal; psi' = 0 is never accepted
  holes = vec.copy()
  start = cfg[:b]
  holes[eo.index(start, top, bot)] = 0.0
  holes[::5] = 0.0
  eng = _engine(n, b, length, (top, bot))
  eng.set_params(holes); eng.set_configs(start)
  cur = start.copy()
  for step in range(6):
    eng.step_counter = step
    pu, pd, _ = eng.debug_proposals(step)
    eng.mc_steps(1)
    got = eng.get_configs()
    new = cur.copy(); new[np.arange(b), pu] = -1.0; new[np.arange(b), pd] = 1.0
    p_old, p_new = holes[eo.index(cur, top, bot)], holes[eo.index(new, top, bot)]
    leave = (p_old == 0) & (p_new != 0)
    stay = p_new == 0
    np.testing.assert_array_equal(got[leave], new[leave])
    np.testing.assert_array_equal(got[stay], cur[stay])
    cur = got
  assert (holes[eo.index(cur, top, bot)] != 0).mean() > 0.9
  eng.close()


def test_edvec_sampler_distribution_chi2_on_a_ring():
  """8-site ring: the sampled frequencies of the 70 Sz = 0 configurations against |v|^2."""
  n, b = 8, 2048
  top, bot, length = eo.lin_tables(n)
  vec = np.random.default_rng(11).standard_normal(length).astype(np.float32)
  all_cfg = eo.sz0_configurations(n)
  w = vec[eo.index(all_cfg, top, bot)].astype(np.float64) ** 2
  w /= w.sum()
  eng = _engine(n, b, length, (top, bot))
  eng.set_params(vec)
  eng.set_configs(vo.random_configurations(n, b, np.random.RandomState(12)))
  eng.mc_steps(200)
  index = {tuple(r.astype(int)): i for i, r in enumerate(all_cfg)}
  counts = np.zeros(len(all_cfg))
  for _ in range(10):
    eng.mc_steps(40)
    for r in eng.get_configs():
      counts[index[tuple(r.astype(int))]] += 1
  expect = w * counts.sum()
  keep = expect > 5
  chi2 = ((counts[keep] - expect[keep]) ** 2 / expect[keep]).sum()
  dof = keep.sum() - 1
  # samples 40 steps apart are not independent: allow a generous factor over the 99.9 % quantile
  assert chi2 < 3.0 * (dof + 3.1 * np.sqrt(2 * dof)), (chi2, dof)
  eng.close()


def _acc_check(res, vec, cfg, top, bot, w, label, extra=0):
  """g1 and g2 against the oracle within (c + 2 + extra) u sum |terms| per entry; returns the chains per entry."""
  p = len(vec)
  g1, g2, a1, a2, cnt = eo.accumulate(vec, cfg, top, bot, w)
  worst = 0.0
  for got, ref, mag in ((res[:p], g1, a1), (res[p:2 * p], g2, a2)):
    bound = (cnt + 2 + extra) * U * mag
    err = np.abs(got.astype(np.float64) - ref)
    assert (err[cnt == 0] == 0).all()
    worst = max(worst, (err[cnt > 0] / bound[cnt > 0]).max())
  print('ed_vector accumulators (%s): worst error / bound = %.3f, up to %d chains per entry' % (label, worst, cnt.max()))
  assert worst <= 1.0, worst
  return cnt


def _collision_run(seed_env, monkeypatch):
  n, b = 8, 256
  bonds = [tuple(x) for x in vo.chain_bonds(n)]
  top, bot, length = eo.lin_tables(n)
  rng = np.random.default_rng(21)
  vec = rng.standard_normal(length).astype(np.float32)
  vec_w = (vec + 0.3 * rng.standard_normal(length)).astype(np.float32)
  cfg = _random_sz0(n, b, 22)
  vec[eo.index(cfg[:3], top, bot)] = 0.0                   # three chains (and their twins) contribute nothing
  monkeypatch.setenv('CGS_VMC_SEED', seed_env)
  eng = _engine(n, b, length, (top, bot))
  eng.set_params(vec); eng.set_configs(cfg); eng.set_bonds(bonds, 1.0, 1.0)
  out = {}
  eloc = eng.local_energy()[0]
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  out['eg'] = eng.get_accumulators()
  eng.set_params(vec_w, _hip.VMC_OMEGA)
  eloc_w = eng.local_energy(_hip.VMC_OMEGA)[0]
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.05)
  out['itswo'] = eng.get_accumulators()
  # three Adam steps from sampled chains (the zero entries are left behind by the sampler)
  for _ in range(3):
    eng.mc_steps(16)
    eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.apply_adam(_hip.VMC_MODE_ENERGY_GRADIENT, 1e-3)
  out['acc3'] = eng.get_accumulators(); out['theta3'] = eng.get_params(); out['chains'] = eng.get_configs()
  eng.close()
  return out, (vec, vec_w, cfg, top, bot, eloc, eloc_w)


def test_edvec_accumulators_with_collisions_and_bit_identical_reruns(monkeypatch):
  """256 chains over 70 entries, both modes.  The weights are the fp32 local energies (pinned by the exact-state test)
  and, for ITSWO, the fp32 ratio formed from them one IEEE operation at a time; the oracle sums in fp64."""
  out, (vec, vec_w, cfg, top, bot, eloc, eloc_w) = _collision_run('31', monkeypatch)
  p = len(vec)
  psi = vec[eo.index(cfg, top, bot)]
  live = psi != 0
  cnt = _acc_check(out['eg'], vec, cfg, top, bot, eloc, 'EnergyGradient')
  assert cnt.max() >= 4 and (cnt > 1).sum() > 20 and not live.all()
  sc = out['eg'][2 * p:]
  assert sc[1] == 256 and sc[4] == 1
  ratio = eo.itswo_ratio_fp32(psi, vec_w[eo.index(cfg, top, bot)], eloc_w, 0.05)
  _acc_check(out['itswo'], vec, cfg, top, bot, ratio, 'LogOverlapITSWO')
  sc = out['itswo'][2 * p:]
  assert sc[1] == 256 and sc[3] == 256 and sc[4] == 1
  # (three chains sit on psi = 0, where the ratio is inf or NaN: the energy and ratio sums of this mode are compared in
  # test_edvec_energy_slots_without_zero_amplitudes)
  assert not np.isfinite(ratio).all()
  again, _ = _collision_run('31', monkeypatch)
  for k in out:
    np.testing.assert_array_equal(out[k].view(np.uint32), again[k].view(np.uint32), err_msg=k)
  assert np.isfinite(out['theta3']).all() and (out['theta3'] != vec).any()


def test_edvec_energy_slots_without_zero_amplitudes():
  """Both modes on a positive vector: every slot is finite.  The sums of a slot are formed in double and rounded once,
  then added to the zeroed slot: within 2 u sum |values| of the fp64 sum of the fp32 values."""
  n, b = 8, 256
  bonds = [tuple(x) for x in vo.chain_bonds(n)]
  top, bot, length = eo.lin_tables(n)
  rng = np.random.default_rng(23)
  vec = rng.uniform(0.5, 1.5, length).astype(np.float32)
  vec_w = (vec + rng.uniform(-0.2, 0.2, length)).astype(np.float32)
  cfg = _random_sz0(n, b, 24)
  eng = _engine(n, b, length, (top, bot))
  eng.set_params(vec); eng.set_configs(cfg); eng.set_bonds(bonds, 1.0, 1.0)
  eloc = eng.local_energy()[0]
  ref = eo.local_energy(vec, cfg, top, bot, bonds, 1.0, 1.0)
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  res = eng.get_accumulators()
  _acc_check(res, vec, cfg, top, bot, eloc, 'positive vector')
  assert abs(res[2 * length] - ref.sum()) <= 16 * U * np.abs(ref).sum() and res[2 * length + 1] == b
  assert abs(res[2 * length] - eloc.astype(np.float64).sum()) <= 2 * U * np.abs(eloc).sum()
  grad = eng.get_gradient(_hip.VMC_MODE_ENERGY_GRADIENT)
  g1, g2, _, _, _ = eo.accumulate(vec, cfg, top, bot, eloc)
  want = g2 - eloc.astype(np.float64).mean() * g1
  assert np.abs(grad - want).max() <= 1e-5 * np.abs(want).max()
  # LogOverlapITSWO: the energy slot sums E_loc of omega, the ratio slot (psi_w / psi)(1 - beta E_loc^w)
  eng.set_params(vec_w, _hip.VMC_OMEGA)
  eloc_w = eng.local_energy(_hip.VMC_OMEGA)[0]
  eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.05)
  res = eng.get_accumulators()
  psi, psi_w = vec[eo.index(cfg, top, bot)], vec_w[eo.index(cfg, top, bot)]
  ratio = eo.itswo_ratio_fp32(psi, psi_w, eloc_w, 0.05)
  assert np.isfinite(ratio).all() and np.isfinite(res).all()
  _acc_check(res, vec, cfg, top, bot, ratio, 'positive vector, LogOverlapITSWO')
  sc = res[2 * length:]
  assert sc[1] == b and sc[3] == b and sc[4] == 1
  assert abs(sc[0] - eloc_w.astype(np.float64).sum()) <= 2 * U * np.abs(eloc_w).sum(), (sc[0], eloc_w.sum())
  assert abs(sc[2] - ratio.astype(np.float64).sum()) <= 2 * U * np.abs(ratio).sum(), (sc[2], ratio.sum())
  eng.close()


def test_edvec_sharded_chains_match_one_ctx():
  """Two ctxs with chain_offset 0 and B/2 against one ctx and the fp64 oracle.  Each side and the single ctx lie within
  case 5's (c + 2) u sum |terms| of the oracle over their own chains; the host sum of the two sides (formed in fp32, as
  an all-reduce forms it) adds one rounding: (c + 3) u sum |terms| with c over both sides."""
  n, b = 8, 256
  bonds = [tuple(x) for x in vo.chain_bonds(n)]
  top, bot, length = eo.lin_tables(n)
  vec = np.random.default_rng(25).standard_normal(length).astype(np.float32)
  cfg = _random_sz0(n, b, 26)
  one = _engine(n, b, length, (top, bot))
  halves = [_engine(n, b // 2, length, (top, bot), chain_offset=r * (b // 2)) for r in range(2)]
  for r, eng in enumerate([one] + halves):
    eng.set_params(vec); eng.set_bonds(bonds, 1.0, 1.0)
    eng.set_configs(cfg if r == 0 else cfg[(r - 1) * (b // 2):r * (b // 2)])
    eng.mc_steps(20)
    eng.reset_accumulators()
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  chains = one.get_configs()
  np.testing.assert_array_equal(np.concatenate([h.get_configs() for h in halves]), chains)
  eloc = one.local_energy()[0]
  np.testing.assert_array_equal(np.concatenate([h.local_energy()[0] for h in halves]).view(np.uint32), eloc.view(np.uint32))
  a = one.get_accumulators()
  sides = [h.get_accumulators() for h in halves]
  _acc_check(a, vec, chains, top, bot, eloc, 'one ctx')
  for r, side in enumerate(sides):
    rows = slice(r * (b // 2), (r + 1) * (b // 2))
    _acc_check(side, vec, chains[rows], top, bot, eloc[rows], 'chains %d..%d' % (rows.start, rows.stop - 1))
  s = sides[0] + sides[1]                                   # fp32: one rounding per entry
  _acc_check(s, vec, chains, top, bot, eloc, 'host sum of the two sides', extra=1)
  p = length
  # the energy slot: each side sums in double and rounds once, the host sum rounds once more
  e64 = eloc.astype(np.float64)
  assert abs(s[2 * p] - e64.sum()) <= 3 * U * np.abs(e64).sum() and abs(a[2 * p] - e64.sum()) <= 2 * U * np.abs(e64).sum()
  assert s[2 * p + 1] == a[2 * p + 1] == b
  for eng in [one] + halves:
    eng.close()


def test_edvec_two_gloo_ranks_match_one_ctx():
  """The multi-rank path: two gloo rank processes on this GPU, half of the chains each (tests/_edvec_gloo_worker.py).
  vmc_allreduce_accumulators against the oracle over all chains at (c + 3) u, then run_optimization_epoch through the
  vmc_epoch_*_dist entries and run_evaluation through vmc_evaluate against an unsharded engine."""
  import socket
  import subprocess
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sock = socket.socket(); sock.bind(('127.0.0.1', 0)); port = sock.getsockname()[1]; sock.close()
  procs = []
  for rank in range(2):
    env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
               MASTER_PORT=str(port), CGS_VMC_DIST_BACKEND='gloo', CGS_VMC_TRANSPORT='host', HSA_ENABLE_IPC_MODE_LEGACY='0')
    procs.append(subprocess.Popen([sys.executable, os.path.join(root, 'tests', '_edvec_gloo_worker.py')],
                                  env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
  outs = []
  for proc in procs:
    try:
      out, _ = proc.communicate(timeout=300)
    except subprocess.TimeoutExpired:
      for q in procs:
        q.kill()
      raise
    outs.append(out.decode())
  for rank, (proc, out) in enumerate(zip(procs, outs)):
    print(''.join(line + '\n' for line in out.splitlines() if 'ed_vector' in line), end='')
    assert proc.returncode == 0 and 'rank {} ok'.format(rank) in out, out[-4000:]


def test_edvec_run_training_and_reload(tmp_path, monkeypatch):
  """run_training --wavefunction_type=ed_vector on the 4 x 4 torus at jx = -1 (Marshall-rotated: E0 = -11.2285) from a
  positive random vector: EnergyGradient (.npz checkpoints) and LogOverlapITSWO (TF bundles), each then --resume_training;
  the energy falls and never undercuts E0 by more than three standard errors; StochasticReconfiguration is refused."""
  from cgs_vmc_amd import run_energy_evaluation, run_training, session, wavefunctions
  from tools import make_ed_vector as mk
  e0 = eo.vector_from_ed(16, _square_bonds(4, 4), -1.0, 1.0)[0]
  files = 'top_lin_table_file=top_lin_table.txt,bot_lin_table_file=bot_lin_table.txt,ed_vector_file=ed_vector.txt'
  hp = ('batch_size=1024,num_equilibration_sweeps=10,num_batches_per_epoch=10,learning_rates=[0.0005,0.0005],'
        'learning_rate_stops=[1000],num_evaluation_samples=20,' + files)
  for fmt, opt, epochs in (('npz', 'EnergyGradient', 30), ('tf', 'LogOverlapITSWO', 10)):
    monkeypatch.setenv('CGS_VMC_CHECKPOINT_FORMAT', fmt)
    d = str(tmp_path / fmt)
    mk.main([d, '--lattice', 'square', '--size', '4', '4', '--random', '--seed', '3'])
    os.remove(os.path.join(d, 'model_prior_0_epochs.npz')); os.remove(os.path.join(d, 'checkpoint'))
    args = ['--checkpoint_dir', d, '--num_sites', '16', '--heisenberg_jx', '-1.0', '--wavefunction_type', 'ed_vector',
            '--optimizer', opt, '--hparams', hp]
    session.reset_default_graph(); wavefunctions.reset_name_scope()
    run_training.main(args + ['--num_epochs', str(epochs)])
    energies = [float(x) for x in open(os.path.join(d, 'metrics.txt')).read().split()]
    assert len(energies) == epochs and np.isfinite(energies).all()
    assert energies[-1] < energies[0], energies
    # --resume_training reloads the last checkpoint of either format and goes on from its energy
    session.reset_default_graph(); wavefunctions.reset_name_scope()
    run_training.main(args + ['--num_epochs', '2', '--resume_training', 'true'])
    resumed = [float(x) for x in open(os.path.join(d, 'metrics.txt')).read().split()][epochs:]
    assert len(resumed) == 2 and resumed[0] < energies[0], (resumed, energies)
    if fmt == 'tf':
      assert not any(f.endswith('.npz') for f in os.listdir(d))
    session.reset_default_graph(); wavefunctions.reset_name_scope()
    samples = run_energy_evaluation.evaluate(run_energy_evaluation.cli_common.parser_from_table(
        '', run_energy_evaluation.FLAG_TABLE).parse_args(['--checkpoint_dir', d, '--heisenberg_jx', '-1.0']))
    mean, se = samples.mean(), samples.std(ddof=1) / np.sqrt(len(samples))
    print('ed_vector 4x4 %s: first epoch E %.4f, last epoch E %.4f, evaluated E %.4f +/- %.4f (exact %.4f)'
          % (opt, energies[0], energies[-1], mean, se, e0))
    assert mean > e0 - 3 * se, (mean, se, e0)
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  with pytest.raises(NotImplementedError):
    run_training.main(['--checkpoint_dir', d, '--num_sites', '16', '--heisenberg_jx', '-1.0',
                       '--wavefunction_type', 'ed_vector', '--optimizer', 'StochasticReconfiguration',
                       '--num_epochs', '2', '--hparams', 'batch_size=64,' + files])
  session.reset_default_graph(); wavefunctions.reset_name_scope()


def test_edvec_life_cycle_and_refusals():
  import torch
  n, b = 8, 32
  bonds = [tuple(x) for x in vo.chain_bonds(n)]
  top, bot, length = eo.lin_tables(n)
  vec = np.ones(length, np.float32)
  eng = _engine(n, b, length)                            # no tables yet
  eng.set_params(vec); eng.set_bonds(bonds, 1.0, 1.0)
  eng.set_configs(_random_sz0(n, b, 27))
  for call in (lambda: eng.amplitude(), lambda: eng.amplitude(_random_sz0(n, 4, 28)), lambda: eng.mc_steps(4),
               lambda: eng.mc_step_injected(np.zeros(b), np.ones(b), np.zeros(b)), lambda: eng.local_energy(),
               lambda: eng.local_energy_terms(), lambda: eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT),
               lambda: eng.evaluate(None, 1, 1, 1)):
    with pytest.raises(ValueError, match='vmc_set_lin_tables'):
      call()
  with pytest.raises(ValueError, match='outside'):
    eng.set_lin_tables(top, bot + 1)
  with pytest.raises(ValueError, match='entries each'):
    eng.set_lin_tables(top[:8], bot[:8])
  eng.set_lin_tables(top, bot)
  assert eng.amplitude()[1].tolist() == [1.0] * b
  eng.close()
  from cgs_vmc_amd.engine import VmcEngine
  other = VmcEngine(n, b, 1, 8)
  with pytest.raises(ValueError, match='not an ed_vector ctx'):
    other.set_lin_tables(top, bot)
  other.close()
  with pytest.raises(ValueError):
    _engine(7, 4, 35)
  with pytest.raises(NotImplementedError):
    _engine(30, 4, 100)
  with pytest.raises(ValueError):
    _engine(n, 4, 0)
  torch.cuda.synchronize()
  free0 = torch.cuda.mem_get_info()[0]
  for _ in range(10):
    e = _engine(n, b, length, (top, bot))
    e.set_params(vec); e.set_bonds(bonds, 1.0, 1.0); e.set_configs(_random_sz0(n, b, 29))
    e.mc_steps(8); e.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    e.close()
  torch.cuda.synchronize()
  assert free0 - torch.cuda.mem_get_info()[0] < (8 << 20)

"""GPU: the product ctx's own kernels (csrc/prod.hip, csrc/vmc_api_prod.hip) off the 4 x 4 torus, against the fp64 product
oracle on the inputs of tests/prod_shape_cases.py (the table there says which path each shape reaches; tests/test_prod.py
proves on the oracle alone that the inputs keep the caps leant on here: banded verdicts, acceptance shares, pbdg logit
bounds below 0.5, the groups of the injected steps).

Tolerances: nothing new.  Each quantity is held to the SUM of its two factors' own test bounds, as in
tests/test_gpu_prod.py (prod_shape_cases.logit_bound / eloc_bound / scalar_rtol):
  logits     dense 2e-5 max(1, |ref|) (tests/test_gpu_random_shapes.py), pbdg 64 (N/2) eps32 kappa(M), ed_vector
             4 eps32 |ln|v|| + eps32
  E_loc      dense 3e-4 max(1, |ref|), pbdg rtol 2e-3 with atol 2e-3 mean|ref|, ed_vector (n_b + 3) 2^-24 (|diag| + sum|terms|)
  g1 / g2    per factor segment: dense 2e-3 max|ref| + 2e-4, pbdg 2e-3 max|ref| + 1e-4 (tests/test_gpu_pbdg.py), summed
             over the two factors because the weights (E_loc, the ITSWO ratio) carry both factors' errors.  The ed_vector
             segment is a gather of w_b / psi_b: per entry (c + 2) 2^-24 sum|w_b / psi_b| (tests/test_gpu_edvec.py's
             _acc_check, c chains on the entry) plus sum |dw_b| / |psi_b| with |dw_b| the bound already asserted on the
             weight (E_loc's, or for the ITSWO ratio |r| (logit bounds of psi and psi_w) + |psi_w / psi| beta (E_loc^w's
             bound)); an ed_vector factor adds nothing to the other factor's segment bound
  accept     chains equal the oracle's replay outside BASELINE.md's band | |psi'/psi| - sqrt(u) | < 1e-4 |psi'/psi|
"""
import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo
from tests import prod_oracle as pro
from tests import prod_shape_cases as psc

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _engine(cid, prod=None):
  from cgs_vmc_amd.engine import VmcEngine
  c = psc.CASES[cid]
  prod = prod or psc.product_of(cid)
  eng = VmcEngine(c['n'], c['b_chains'], 0, 0, ansatz='prod', children=psc.specs(cid), seed=psc.SEED,
                  chain_offset=c['offset'])
  assert eng.kernel_path() == 10 and eng.num_params == prod.num_params
  theta = np.concatenate([prod.a.theta, prod.b.theta]).astype(np.float32)
  eng.set_params(theta)
  np.testing.assert_array_equal(eng.get_params(), theta)
  bonds, jx, jz = psc.bonds(cid)
  eng.set_bonds(bonds, jx, jz)
  return eng, prod


def _worst(what, err, bound):
  err, bound = np.atleast_1d(err), np.atleast_1d(bound)
  with np.errstate(divide='ignore', invalid='ignore'):
    q = np.where(err == 0, 0.0, err / bound)
  k = int(np.argmax(q))
  print('%s: max error %.3g, worst error / bound %.4f (error %.3g, bound %.3g)' % (what, err.max(), q[k], err[k], bound[k]))
  assert (err <= bound).all(), (what, err[k], bound[k])


def _bits(x):
  return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize('cid', psc.IDS)
def test_amplitudes_and_local_energies_match_the_oracle(cid):
  eng, prod = _engine(cid)
  cfg = psc.start(cid)
  bonds, jx, jz = psc.bonds(cid)
  eng.set_configs(cfg)
  logit, psi = eng.amplitude(cfg)
  ref = prod.psi(cfg)
  bound = psc.logit_bound(prod, cfg)
  _worst('%s logit' % cid, np.abs(logit.astype(np.float64) - np.log(np.abs(ref))), bound)
  sure = bound < 0.5
  assert sure.all()                                         # (tests/test_prod.py: the inputs keep it so)
  np.testing.assert_array_equal(np.sign(psi)[sure], np.sign(ref)[sure])
  if psc.signed(cid) and len(cfg) > 4:
    assert (ref > 0).any() and (ref < 0).any()
  np.testing.assert_allclose(np.abs(psi), np.exp(logit.astype(np.float64)), rtol=1e-5, atol=1e-37)
  lc, pc = eng.amplitude()                                  # the chains' cache: bit for bit
  np.testing.assert_array_equal(_bits(lc), _bits(logit)); np.testing.assert_array_equal(_bits(pc), _bits(psi))
  e, mean = eng.local_energy()
  e_ref = prod.local_energy(cfg, bonds, jx, jz)
  _worst('%s E_loc' % cid, np.abs(e - e_ref), psc.eloc_bound(prod, cfg, e_ref, bonds, jx, jz))
  assert abs(mean - e.astype(np.float64).mean()) <= 1e-5 * np.abs(e).mean() + 1e-6
  d, o = eng.local_energy_terms()
  np.testing.assert_allclose(d + o, e, rtol=1e-6, atol=1e-6)
  d_ref = sum(0.25 * float(z) * cfg[:, i].astype(np.float64) * cfg[:, j] for (i, j), z in zip(bonds, jz))
  np.testing.assert_allclose(d, d_ref, rtol=0, atol=16 * U * len(bonds))
  assert eng.last_connected_rows() == int(sum((cfg[:, i] != cfg[:, j]).sum() for i, j in bonds))    # repeats counted
  eng.close()


@pytest.mark.parametrize('cid', psc.ROW_BLOCK_CASES)
def test_host_rows_in_blocks_equal_full_blocks_bit_for_bit(cid):
  """amplitude(rows) walks host rows in blocks of B; a short last block repeats its first row.  Every row must come out
  as it does at the same position of a full B-row call."""
  eng, prod = _engine(cid)
  b = psc.CASES[cid]['b_chains']
  rows = psc.pool(cid)
  assert len(rows) == 2 * b + 3
  ref_l, ref_p = np.empty(len(rows), np.float32), np.empty(len(rows), np.float32)
  for r0 in range(0, len(rows), b):
    n = min(b, len(rows) - r0)
    block = np.concatenate([rows[r0:r0 + n], rows[:b - n]])         # a full call: the tail filled with other rows
    l, p = eng.amplitude(block)
    ref_l[r0:r0 + n], ref_p[r0:r0 + n] = l[:n], p[:n]
  want = prod.psi(rows)
  _worst('%s host-row logit' % cid, np.abs(ref_l.astype(np.float64) - np.log(np.abs(want))), psc.logit_bound(prod, rows))
  np.testing.assert_array_equal(np.sign(ref_p), np.sign(want))
  for n_rows in (1, b - 1, b + 1, 2 * b + 3):
    l, p = eng.amplitude(rows[:n_rows])
    np.testing.assert_array_equal(_bits(l), _bits(ref_l[:n_rows]), err_msg='n_rows = %d' % n_rows)
    np.testing.assert_array_equal(_bits(p), _bits(ref_p[:n_rows]), err_msg='n_rows = %d' % n_rows)
  if psc.signed(cid):
    bad = rows[:b + 1].copy()
    bad[b, np.flatnonzero(bad[b] < 0)[0]] = 1.0                     # Sz != 0 in the short second block
    with pytest.raises(ValueError):
      eng.amplitude(bad)
    l, p = eng.amplitude(rows[:b + 1])                              # ... and the ctx still works
    np.testing.assert_array_equal(_bits(l), _bits(ref_l[:b + 1]))
  eng.close()


@pytest.mark.parametrize('cid', ['S1', 'S3', 'S4', 'S6'])
def test_proposals_are_the_oracles_philox_with_offset_chain_ids(cid):
  eng, _ = _engine(cid)
  c = psc.CASES[cid]
  cfg = psc.start(cid)
  eng.set_configs(cfg)
  for step in (0, 7, 2 ** 33 + 1):
    i_up, i_dn, u = eng.debug_proposals(step)
    r_up, r_dn, r_u = psc.proposals(cid, cfg, step)
    np.testing.assert_array_equal(i_up, r_up); np.testing.assert_array_equal(i_dn, r_dn)
    np.testing.assert_array_equal(_bits(u), _bits(r_u))
    plain_u = vo.step_uniforms(psc.SEED, np.arange(c['b_chains']), step, c['n'])[1]     # (without the offset: other draws)
    assert c['offset'] == 0 or not np.array_equal(u, plain_u)
  np.testing.assert_array_equal(eng.get_configs(), cfg)
  eng.close()


@pytest.mark.parametrize('cid', psc.IDS)
def test_mc_steps_replayed_by_the_oracle(cid):
  """mc_steps(n): step 0's proposal is k_wide_propose's, steps 1 .. n-1 are drawn by k_prod_accept's own copy of the rule
  from the spins as patched after its commit.  The oracle replays with its own Philox (offset chain ids) and
  pro.mc_step's verdicts: the chains must equal the replay on every chain without a banded verdict, and where no chain
  was banded (tests/test_prod.py: S5 has none) the returned count is the oracle's -- k_prod_count_fold's sum."""
  eng, prod = _engine(cid)
  c = psc.CASES[cid]
  eng.set_configs(psc.start(cid))
  assert eng.step_counter == 0
  accepted = eng.mc_steps(c['steps'])
  assert eng.step_counter == c['steps']
  rep = psc.replay(cid)
  got = eng.get_configs()
  print('%s: %d steps, accepted %d (oracle %d, share %.3f), banded chains %d' % (
      cid, c['steps'], accepted, rep.accepted, rep.share, rep.band.sum()))
  assert rep.band.sum() <= 2
  np.testing.assert_array_equal(got[~rep.band], rep.configs[~rep.band])
  if not rep.band.any():
    assert accepted == rep.accepted
  assert (got.sum(1) == 0).all() and (np.abs(got) == 1).all()
  lc, pc = eng.amplitude()
  lr, pr = eng.amplitude(got)
  np.testing.assert_array_equal(_bits(lc), _bits(lr)); np.testing.assert_array_equal(_bits(pc), _bits(pr))
  eng.close()


def test_evaluate_counts_the_oracles_accepts_over_its_samples():
  """S1: evaluate(None, n_eq, 3, n_mc) sums mc_steps' counts over the measurement sweeps (the equilibration is not
  counted), and its means are the local energies of the replayed chains."""
  cid, e = 'S1', psc.EVAL
  eng, prod = _engine(cid)
  bonds, jx, jz = psc.bonds(cid)
  eng.set_configs(psc.start(cid))
  means, accepted = eng.evaluate(None, e['n_eq'], e['n_samples'], e['n_mc'])
  eq, samples = psc.eval_replay()
  assert not eq.band.any() and not any(s.band.any() for s in samples)       # (tests/test_prod.py)
  assert accepted == sum(s.accepted for s in samples)
  assert eng.step_counter == e['n_eq'] + e['n_samples'] * e['n_mc']
  np.testing.assert_array_equal(eng.get_configs(), samples[-1].configs)
  chains = [eq.configs] + [s.configs for s in samples[:-1]]
  for k, cfg in enumerate(chains):
    ref = prod.local_energy(cfg, bonds, jx, jz)
    _worst('S1 evaluate mean %d' % k, abs(means[k] - ref.mean()), psc.eloc_bound(prod, cfg, ref, bonds, jx, jz).mean())
  eng.close()


@pytest.mark.parametrize('name', sorted(psc.SCRIPTS))
def test_injected_steps_with_bad_and_zero_moves(name):
  """A proposal whose i_up names a down site or whose i_dn names an up site: mask false, chain unchanged (the host
  checks the index range only; k_prod_candidates and k_prod_accept guard the spins).  A chain on psi = 0 accepts its
  first non-zero candidate; a candidate on a zero is rejected.  Masks and chains equal pro.mc_step's throughout."""
  s = psc.SCRIPTS[name]()
  eng, prod = _engine(s.cid, s.prod)
  eng.set_configs(s.start)
  _, psi = eng.amplitude()
  np.testing.assert_array_equal(psi == 0, prod.psi(s.start) == 0)
  assert (psi == 0).sum() >= 2
  for k, (i_up, i_dn, u) in enumerate(s.steps):
    mask = eng.mc_step_injected(i_up, i_dn, u)
    np.testing.assert_array_equal(mask, s.masks[k], err_msg='step %d' % k)
    np.testing.assert_array_equal(eng.get_configs(), s.after[k], err_msg='step %d' % k)
  assert s.zero_start >= 2 and s.zero_cand >= 2 and s.bad >= 2 and not s.band.any()     # (tests/test_prod.py)
  lc, pc = eng.amplitude()
  lr, pr = eng.amplitude(s.after[-1])
  np.testing.assert_array_equal(_bits(lc), _bits(lr)); np.testing.assert_array_equal(_bits(pc), _bits(pr))
  eng.close()


# ---- accumulators
def _segment_bounds(prod, ref_a, ref_b):
  """Per factor segment: the two factors' own g-sum bounds, summed (None for an ed_vector segment: _edvec_segment)."""
  def own(f, ref):
    if f.kind == 'ed_vector':
      return 0.0
    return 2e-3 * np.abs(ref).max() + (1e-4 if f.kind == 'pbdg' else 2e-4)
  return (None if prod.a.kind == 'ed_vector' else own(prod.a, ref_a) + own(prod.b, ref_a),
          None if prod.b.kind == 'ed_vector' else own(prod.a, ref_b) + own(prod.b, ref_b))


def _edvec_segment(what, got, vec, cfg, w_ref, w_bound, keep, g2):
  """The ed_vector factor's segment: entry k holds sum_b [idx_b = k] w_b / v_k (w = 1 for g1)."""
  top, bot, _ = eo.lin_tables(cfg.shape[1])
  idx = eo.index(cfg, top, bot)
  psi = np.asarray(vec, np.float64)[idx]
  live = (keep if g2 else np.ones(len(cfg), bool)) & (psi != 0)       # (keep: the chains whose weight is not exactly 0)
  w = np.where(live, w_ref, 0.0) if g2 else live.astype(np.float64)
  ref, mag, cnt, slack = (np.zeros(len(vec)) for _ in range(4))
  np.add.at(ref, idx[live], w[live] / psi[live])
  np.add.at(mag, idx[live], np.abs(w[live] / psi[live]))
  np.add.at(cnt, idx[live], 1.0)
  if g2:
    np.add.at(slack, idx[live], w_bound[live] / np.abs(psi[live]))
  err = np.abs(got.astype(np.float64) - ref)
  assert (err[cnt == 0] == 0).all(), what
  _worst(what, err[cnt > 0], ((cnt + 2) * U * mag + slack)[cnt > 0])


def _check_accumulators(cid, tag, res, prod, cfg, g1, g2, w_ref, w_bound, keep=None):
  pa, p = prod.a.num_params, prod.num_params
  keep = np.ones(len(cfg), bool) if keep is None else keep
  assert np.isfinite(res[:2 * p]).all()
  for which, (got, ref) in enumerate(((res[:p], g1), (res[p:2 * p], g2))):
    bounds = _segment_bounds(prod, ref[:pa], ref[pa:])
    for f, sl, bound, seg in ((prod.a, slice(0, pa), bounds[0], 'a'), (prod.b, slice(pa, p), bounds[1], 'b')):
      what = '%s %s g%d_%s (%s)' % (cid, tag, which + 1, seg, f.kind)
      if f.kind == 'ed_vector':
        _edvec_segment(what, got[sl], f.theta, cfg, w_ref, w_bound, keep, which == 1)
      else:
        _worst(what, np.abs(got[sl] - ref[sl]).max(), bound)


def _check_gradient(cid, tag, got, ref, prod):
  """The final gradient per factor segment, at tests/test_gpu_prod.py's bound: 2e-3 max|ref| + 2e-4 per factor.  (An
  ed_vector segment has no bound of its own for it in tests/test_gpu_edvec.py beyond the sums checked above.)"""
  pa = prod.a.num_params
  assert np.isfinite(got).all()
  for f, sl, seg in ((prod.a, slice(0, pa), 'a'), (prod.b, slice(pa, None), 'b')):
    if f.kind != 'ed_vector':
      _worst('%s %s gradient_%s (%s)' % (cid, tag, seg, f.kind), np.abs(got[sl] - ref[sl]).max(),
             2 * (2e-3 * np.abs(ref[sl]).max() + 2e-4))


@pytest.mark.parametrize('cid', ['S1', 'S2', 'S3', 'S4'])
def test_accumulators_of_both_modes_match_the_oracle(cid):
  eng, prod = _engine(cid)
  cfg = psc.start(cid)
  bonds, jx, jz = psc.bonds(cid)
  b, p = len(cfg), prod.num_params
  eng.set_configs(cfg)
  rtol = psc.scalar_rtol(prod)
  # EnergyGradient
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  acc = vo.Accumulators(p, np.float64)
  e_ref = pro.energy_gradient_accumulate(acc, prod, cfg, bonds, jx, jz)
  e_bound = psc.eloc_bound(prod, cfg, e_ref, bonds, jx, jz)
  res = eng.get_accumulators()
  _check_accumulators(cid, 'EnergyGradient', res, prod, cfg, acc.g1_total, acc.g2_total, e_ref, e_bound)
  # scalar slots: the relative bounds of tests/test_gpu_prod.py; an ed_vector factor adds the sum of its own per-row bounds
  ed_abs = psc.eloc_bound(prod, cfg, e_ref, bonds, jx, jz, only='ed_vector').sum()
  _worst('%s e_total' % cid, abs(res[2 * p] - acc.e_total), rtol * max(1, abs(acc.e_total)) + ed_abs)
  assert res[2 * p + 1] == b and res[2 * p + 4] == 1
  _check_gradient(cid, 'EnergyGradient', eng.get_gradient(_hip.VMC_MODE_ENERGY_GRADIENT), vo.energy_gradient(acc), prod)
  # LogOverlapITSWO with a perturbed supervisor: ratios of both signs where a factor is signed
  beta = 0.05
  wa, wb = psc.omega_thetas(cid)
  eng.set_params(np.concatenate([wa, wb]), _hip.VMC_OMEGA)
  omega = psc.product_of(cid, wa, wb)
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, beta)
  acc = vo.Accumulators(p, np.float64)
  ew_ref, ratio = pro.log_overlap_accumulate(acc, prod, omega, cfg, bonds, jx, jz, beta)
  if psc.signed(cid):
    assert (ratio > 0).any() and (ratio < 0).any()
  ew_bound = psc.eloc_bound(omega, cfg, ew_ref, bonds, jx, jz)
  r_bound = (np.abs(ratio) * (psc.logit_bound(prod, cfg) + psc.logit_bound(omega, cfg) + 8 * U) +
             np.abs(omega.psi(cfg) / prod.psi(cfg)) * beta * ew_bound)
  res = eng.get_accumulators()
  _check_accumulators(cid, 'ITSWO', res, prod, cfg, acc.g1_total, acc.g2_total, ratio, r_bound)
  ed_ew = psc.eloc_bound(omega, cfg, ew_ref, bonds, jx, jz, only='ed_vector')
  ed_r = (np.abs(ratio) * (psc.logit_bound(prod, cfg, 'ed_vector') + psc.logit_bound(omega, cfg, 'ed_vector')) +
          np.abs(omega.psi(cfg) / prod.psi(cfg)) * beta * ed_ew)
  _worst('%s itswo e_total' % cid, abs(res[2 * p] - acc.e_total), rtol * max(1, abs(acc.e_total)) + ed_ew.sum())
  _worst('%s itswo r_total' % cid, abs(res[2 * p + 2] - acc.r_total), rtol * max(1, np.abs(ratio).sum()) + ed_r.sum())
  assert res[2 * p + 1] == b and res[2 * p + 3] == b and res[2 * p + 4] == 1
  _check_gradient(cid, 'ITSWO', eng.get_gradient(_hip.VMC_MODE_LOG_OVERLAP_ITSWO), vo.log_overlap_gradient(acc), prod)
  eng.close()


def test_itswo_with_a_zero_supervisor_entry_follows_the_products_rule():
  """S3, the supervisor's vector zero under chains 0 and 1: k_prod_itswo_ratio gives ratio exactly 0 there (the
  reference, training.py, gives -beta (H psi_w) / psi; the single ed_vector ctx's k_edvec_itswo_ratio NaN).  So every g1 /
  g2 entry is finite, g1 counts all chains, and g2 and the ratio sum are the oracle's with those two chains left out.
  (E_loc of omega is x / 0 on those chains: the energy slot is not finite, as for the factor alone.)"""
  cid, beta = 'S3', 0.05
  eng, prod = _engine(cid)
  cfg = psc.start(cid)
  bonds, jx, jz = psc.bonds(cid)
  p, n = prod.num_params, psc.CASES[cid]['n']
  top, bot, _ = eo.lin_tables(n)
  wa, wb = psc.omega_thetas(cid)
  wb = wb.copy()
  idx = eo.index(cfg, top, bot)
  wb[idx[:2]] = 0.0
  keep = ~np.isin(idx, idx[:2])
  assert (~keep).sum() == 2
  omega = psc.product_of(cid, wa, wb)
  eng.set_configs(cfg)
  eng.set_params(np.concatenate([wa, wb]), _hip.VMC_OMEGA)
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, beta)
  res = eng.get_accumulators()
  assert np.isfinite(res[:2 * p]).all()
  o = prod.log_grads(cfg)
  p_w = omega.psi(cfg)
  with np.errstate(divide='ignore', invalid='ignore'):
    h_psi_w = vo.apply_in_place(omega.psi, cfg, bonds, jx, jz, p_w, np.float64)
    ratio = np.where(keep, (p_w - beta * h_psi_w) / prod.psi(cfg), 0.0)
    ew_ref = np.where(keep, h_psi_w / p_w, 0.0)
  ew_bound, lw = np.zeros(len(cfg)), np.zeros(len(cfg))
  ew_bound[keep] = psc.eloc_bound(omega, cfg[keep], ew_ref[keep], bonds, jx, jz)
  lw[keep] = psc.logit_bound(omega, cfg[keep])
  r_bound = np.abs(ratio) * (psc.logit_bound(prod, cfg) + lw + 8 * U) + np.abs(p_w / prod.psi(cfg)) * beta * ew_bound
  g1 = o.sum(0)
  g2 = (ratio[:, None] * o).sum(0)
  _check_accumulators(cid, 'ITSWO, zero supervisor entry', res, prod, cfg, g1, g2, ratio, r_bound)
  ed_r = (np.abs(ratio) * (psc.logit_bound(prod, cfg, 'ed_vector') + 4 * psc.EPS32 * np.abs(np.log(np.abs(np.where(keep, wb[idx], 1.0)))) + psc.EPS32) +
          np.abs(p_w / prod.psi(cfg)) * beta * np.where(keep, psc.edvec_eloc_bound(wb, cfg, bonds, jx, jz), 0.0))
  _worst('S3 zero supervisor r_total', abs(res[2 * p + 2] - ratio.sum()),
         psc.scalar_rtol(prod) * max(1, np.abs(ratio).sum()) + ed_r.sum())
  assert res[2 * p + 3] == len(cfg) and not np.isfinite(res[2 * p])
  eng.close()

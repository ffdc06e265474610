"""GPU: the symmetrized ctx's own kernels (csrc/symz.hip) past the 8-site chain and the 4 x 4 torus of
tests/test_gpu_symmetrized.py.  The inputs -- lattices, op sets, sectors, seeds -- live in tests/symmetrized_shape_cases.py,
where each shape says which path of which kernel it reaches; tests/test_symmetrized.py proves on the fp64 oracle alone
what is taken for granted here (the ops are symmetries, the fold identity, the seed table's min_c r >= 0.01, the band share).

Tolerances.  Sections 1, 2, 5 and 6 use tests/test_gpu_symmetrized.py's: the base family's own tau (2e-4 dense, 2e-3 pbdg,
(n_b + 3) 2^-24 ed_vector) on cancellation-scaled quantities, |S_gpu - S_ref| <= tau A_ref and r |E_gpu - E_ref| <=
tau max(1, max|E_ref|); min_c r max|g - g_ref| <= 4e-3 max|g_ref| + 2e-4 on the gradient sums.  Section 3 (the in-kernel
proposal draw against k_wide_propose's) has none: bits.  Section 4 separates symz_sum from the base's arithmetic -- the
base's own fp32 logits go through a host fold in fp64 -- and carries a derived bound:
  |logit_gpu - ref| <= 2^-23 max(1, |ref|) + 2^-40 / r
one rounding of m + ln|S| to fp32 (2^-24 relative) with a factor 2 to spare, plus the fp64 sum's error, 2^-43 A over at most
1,024 terms (plan.hpp, PLAN_SYMZ_ZERO) with the zero rule's margin 2^-40, carried through ln: d ln|S| = dS / |S| = 2^-40 A / |S|.
It holds as stated while the base's shift is 0 -- the composite subtracts the shift in fp32, a second rounding at the
magnitude of the raw logit --, so section 4 runs its bases at shift 0 and keeps the logits in range with the output bias.
"""
import json
import os

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import prod_oracle as pro
from tests import symmetrized_oracle as so
from tests import symmetrized_shape_cases as sc
from tests.test_gpu_symmetrized import _base

pytestmark = pytest.mark.gpu
MODE = _hip.VMC_MODE_ENERGY_GRADIENT
COUPLING_SETS = ((1.0, 1.0), (-1.0, 1.0), (0.7, 1.3))


def _compose(base, fac, tau, lat, perms, flips, chi, b, bonds=True):
  from cgs_vmc_amd.engine import VmcEngine
  L = sc.LATTICES[lat]
  if tau is None:
    tau = (len(L['bonds']) + 3) * 2.0 ** -24
  eng = VmcEngine.create_symmetrized(base, b, perms, flips, chi)
  assert eng.kernel_path() == _hip.PATH_SYMMETRIZED and eng.num_params == fac.num_params and eng.children == (base,)
  if bonds:
    eng.set_bonds(L['bonds'], *sc.couplings(lat))
  return eng, so.Symmetrized(fac, perms, flips, chi), tau


def _make(kind, lat, sector, b, seed=0, bonds=True, **kw):
  """(engine, oracle, tau) of a named sector of a lattice of the cases module (tests/test_gpu_symmetrized.py's _make there)."""
  perms, flips, chi = sc.ops(lat, sector)
  base, fac, tau = _base(kind, sc.LATTICES[lat]['n'], b * len(perms), seed, **kw)
  return _compose(base, fac, tau, lat, perms, flips, chi, b, bonds)


def _num_cus():
  import torch
  return int(torch.cuda.get_device_properties(0).multi_processor_count)      # (vmc_create reads the same property)


def _connected(orc, cfg, bonds):
  rows = orc.rows(cfg).reshape(-1, cfg.shape[1])
  return int(sum((rows[:, i] != rows[:, j]).sum() for i, j in bonds))


def _check_amplitudes(eng, orc, cfg, tau, what):
  logit, psi = eng.amplitude(cfg)
  s_ref, a_ref = orc.psi(cfg), orc.A(cfg)
  err = np.abs(psi.astype(np.float64) - s_ref) / a_ref
  print('%s: %d rows, max |S_gpu - S_ref| / A = %.3g (tau %.3g), min r = %.3g' % (
      what, len(cfg), err.max(), tau, (np.abs(s_ref) / a_ref).min()))
  assert (err <= tau).all()
  alive = psi != 0
  np.testing.assert_allclose(np.abs(psi[alive]), np.exp(logit[alive].astype(np.float64)), rtol=2e-6)
  assert np.isneginf(logit[~alive]).all()
  return logit, psi


def _check_local_energies(eng, orc, cfg, lat, tau, what, sets=COUPLING_SETS):
  L = sc.LATTICES[lat]
  r = orc.cancellation(cfg)
  for jx, jz in sets:
    bx, bz = sc.couplings(lat, jx, jz)
    eng.set_bonds(L['bonds'], bx, bz)
    e, mean = eng.local_energy()
    ref = orc.local_energy(cfg, L['bonds'], bx, bz)
    err = r * np.abs(e - ref)
    bound = tau * max(1.0, np.abs(ref).max())
    print('%s jx=%g jz=%g: max r |E - E_ref| = %.3g (bound %.3g), min r = %.3g' % (what, jx, jz, err.max(), bound, r.min()))
    assert (err <= bound).all()
    assert abs(mean - e.astype(np.float64).mean()) < 1e-5 * max(1.0, np.abs(e).max())
    d, o = eng.local_energy_terms()
    np.testing.assert_allclose(d + o, e, rtol=1e-5, atol=1e-5)
    assert eng.last_connected_rows() == _connected(orc, cfg, L['bonds'])


# ---- 1. amplitudes and local energies at the new shapes

@pytest.mark.parametrize('kind,lat,sector,b', sc.AMPLITUDE_CASES)
def test_amplitudes_and_local_energies_at_the_new_shapes(kind, lat, sector, b):
  n = sc.LATTICES[lat]['n']
  eng, orc, tau = _make(kind, lat, sector, b, chain_offset=7)
  what = '%s %s %s B=%d n_ops=%d' % (kind, lat, sector, b, orc.n_ops)
  _check_amplitudes(eng, orc, sc.configs(n, 3 * b + 2, sc.AMPLITUDE_SEED), tau, what)      # host rows: several blocks, a short last one
  # own chains: nothing left out but structural zeros; the same bits as host rows and on a second call
  own = sc.configs(n, b, sc.ELOC_SEED, orc)
  eng.set_configs(own)
  l1, p1 = eng.amplitude()
  l2, p2 = _check_amplitudes(eng, orc, own, tau, what + ' own')
  l3, p3 = eng.amplitude()
  for x, y in ((l1, l2), (p1, p2), (l1, l3), (p1, p3)):
    np.testing.assert_array_equal(x, y)
  _check_local_energies(eng, orc, own, lat, tau, what)
  eng.close()


# ---- 2. two workgroups of the folds, two trips of the row kernels' grid-stride loops

def test_more_rows_than_the_row_grid_and_more_chains_than_a_fold_workgroup():
  big = sc.BIG
  lat, sector, b = big['lat'], big['sector'], big['b']
  n, n_ops = sc.LATTICES[lat]['n'], len(sc.ops(lat, sector)[0])
  # k_symm_rows and k_symz_candidates hold 16 blocks of 4 items per CU: past that their loops take a second trip
  assert n_ops * b > sc.ROW_ITEMS_PER_CU * _num_cus(), (n_ops * b, _num_cus())
  assert sc.FOLD_THREADS < b and b % sc.FOLD_THREADS == 4            # two fold workgroups, the second with four live threads
  assert n > 64
  eng, orc, tau = _make('fc2x16', lat, sector, b)
  what = 'fc2x16 %s %s B=%d' % (lat, sector, b)
  cfg = sc.configs(n, b, big['seed'], orc)
  eng.set_configs(cfg)
  l_own, p_own = eng.amplitude()
  l_host, p_host = _check_amplitudes(eng, orc, cfg, tau, what + ' own')
  np.testing.assert_array_equal(l_own, l_host); np.testing.assert_array_equal(p_own, p_host)
  _check_amplitudes(eng, orc, sc.configs(n, 2 * b + 3, big['seed'] + 1), tau, what + ' host rows')
  _check_local_energies(eng, orc, cfg, lat, tau, what, sets=COUPLING_SETS[:1])
  # one injected step: verdicts agree outside the band, which the oracle alone keeps below its share
  i_up, i_dn, u = sc.big_step(cfg)
  new, acc, ratio = pro.mc_step(orc, cfg, i_up, i_dn, u)
  band = ~(np.abs(ratio ** 2 - u.astype(np.float64)) > tau)
  assert band.sum() <= sc.BAND_SHARE * b
  mask = eng.mc_step_injected(i_up, i_dn, u)
  assert (mask[~band] == acc[~band]).all()
  assert 0 < mask.sum() < b
  cur = np.where(mask[:, None], new, cfg)
  np.testing.assert_array_equal(eng.get_configs(), cur)
  np.testing.assert_array_equal(eng.amplitude()[0], eng.amplitude(cur)[0])
  # three free steps (the in-kernel draw over two workgroups' worth of chains): the cache is vmc_amplitude's, bit for bit
  accepted = eng.mc_steps(3)
  assert 0 < accepted <= 3 * b and (eng.get_configs().sum(1) == 0).all()
  lc, pc = eng.amplitude()
  lr, pr = eng.amplitude(eng.get_configs())
  np.testing.assert_array_equal(lc, lr); np.testing.assert_array_equal(pc, pr)
  eng.close()


# ---- 3. the in-kernel proposal draw is k_wide_propose's

DRAW_PARAMS = [(lat, sector, offset, 0) for lat, sector in sc.DRAW_CASES for offset in sc.DRAW_OFFSETS] + \
    [('chain70', 'q35', 11, sc.HIGH_STEP)]                 # (once with the high word of the step in use)


@pytest.mark.parametrize('lat,sector,offset,step0', DRAW_PARAMS)
def test_the_in_kernel_draw_is_the_proposal_kernels(lat, sector, offset, step0):
  """mc_steps(4) draws the proposals of steps 1 .. 3 inside k_symz_accept; the twin takes every one from k_wide_propose
  (debug_proposals) and injects it.  The same chains, cached logits and count, bit for bit."""
  n, b = sc.LATTICES[lat]['n'], 5
  if lat == 'chain70':
    assert n % 4 != 0 and n > 64                           # a ragged last Philox block, beyond one block per lane's first site
  if lat == 'chain258':
    assert (n + 3) // 4 > 64 and n % 4 != 0                # lane 0 takes a second trip, to a block of two sites
  eng, orc, _ = _make('fc2x16', lat, sector, b, chain_offset=offset)
  twin, _, _ = _make('fc2x16', lat, sector, b, chain_offset=offset)
  cfg = sc.configs(n, b, sc.DRAW_SEED, orc)
  for e in (eng, twin):
    e.set_configs(cfg)
    e.step_counter = step0
  accepted = eng.mc_steps(4)
  total, seen = 0, []
  for step in range(4):
    i_up, i_dn, u = twin.debug_proposals(twin.step_counter)
    rows = twin.get_configs()
    assert (rows[np.arange(b), i_up] > 0).all() and (rows[np.arange(b), i_dn] < 0).all()
    total += int(twin.mc_step_injected(i_up, i_dn, u).sum())
    twin.step_counter = twin.step_counter + 1
    seen.append((i_up, i_dn))
  assert eng.step_counter == twin.step_counter == step0 + 4
  assert any((seen[0][0] != s[0]).any() or (seen[0][1] != s[1]).any() for s in seen[1:])      # (the draws do differ by step)
  np.testing.assert_array_equal(eng.get_configs(), twin.get_configs())
  for x, y in zip(eng.amplitude(), twin.amplitude()):
    np.testing.assert_array_equal(x, y)
  assert accepted == total and accepted > 0
  twin.close(); eng.close()


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tie_events.json')) as f:
  _TIES = json.load(f)
# (lattice, event of tests/golden/tie_events.json): the largest site uniform of that chain and step occurs at two sites,
# both inside the lattice and in Philox blocks of different lanes
TIE_CASES = [('chain8', 2), ('chain70', 1), ('chain70', 2), ('chain258', 3)]


@pytest.mark.parametrize('spin', [1.0, -1.0])
@pytest.mark.parametrize('lat,event', TIE_CASES)
def test_tied_uniforms_in_the_in_kernel_draw_pick_the_first_site(lat, event, spin):
  """tests/test_gpu_ties.py's fixture on k_symz_accept's draw: where two up (down) sites draw the same largest uniform,
  argmax (argmin) of s u picks the smaller index -- across lanes, the `ih < idx_hi` of the shuffle reduction.  All
  parameters zero and the trivial sector: psi_s is constant, every proposal is accepted, and the chains after mc_steps(2)
  -- whose second proposal is drawn in the kernel -- show both proposals, which must equal the oracle's."""
  ev = _TIES['events'][event]
  n, chain, step, sites = sc.LATTICES[lat]['n'], ev['chain'], ev['step'], ev['sites']
  assert _TIES['seed'] == sc.SEED and max(sites) < n and sites[0] // 4 % 64 != sites[1] // 4 % 64
  b, k = 5, 2                                              # the chain sits at row 2 of the batch
  offset, ids = chain - k, np.arange(b, dtype=np.uint32) + np.uint32(chain - k)
  u0, a0 = vo.step_uniforms(sc.SEED, ids, step - 1, n)
  u1, a1 = vo.step_uniforms(sc.SEED, ids, step, n)
  assert u1[k, sites[0]] == u1[k, sites[1]] == u1[k].max()      # the fixture is what it says
  assert (a0 < 1.0).all() and (a1 < 1.0).all()
  # a start row that has `spin` on both tied sites once the move of the step before is made
  rng = np.random.RandomState(chain)
  cfg = vo.random_configurations(n, b, np.random.RandomState(step))
  rows = np.arange(b)
  for attempt in range(200):
    cfg[k] = vo.random_configurations(n, 1, rng)[0]
    first = vo.propose_exchange(cfg, u0)
    want = cfg.copy()
    want[rows, first[1]] = 1.0; want[rows, first[0]] = -1.0
    if (want[k, sites] == spin).all():
      break
  assert (want[k, sites] == spin).all() and (cfg.sum(1) == 0).all() and (want.sum(1) == 0).all()
  second = vo.propose_exchange(want, u1)
  assert (second[0][k] if spin > 0 else second[1][k]) == min(sites)      # the oracle: the first index
  want[rows, second[1]] = 1.0; want[rows, second[0]] = -1.0
  eng, orc, _ = _make('fc2x16', lat, 'q0', b, chain_offset=offset)
  eng.set_params(np.zeros(eng.num_params, np.float32))
  eng.set_configs(cfg)
  eng.step_counter = step - 1
  accepted = eng.mc_steps(2)
  got = eng.get_configs()
  eng.close()
  assert accepted == 2 * b
  np.testing.assert_array_equal(got, want)


# ---- 4. the fold against a host fold of the base's own bits

@pytest.mark.parametrize('factor', list(sc.FOLD_FACTORS))
@pytest.mark.parametrize('lat,sector', sc.FOLD_CASES)
def test_the_fold_of_the_bases_own_logits(lat, sector, factor):
  n, b = sc.LATTICES[lat]['n'], 5
  perms, flips, chi = sc.ops(lat, sector)
  cfg = sc.configs(n, b, sc.FOLD_SEED)
  # the output bias keeps the largest logit of the n_ops B rows at 0: exp(logit) of every fold stays in fp32's range
  bare = sc.fold_theta(n, factor)
  orc = sc.fc_oracle(lat, sector, bare)
  theta = sc.fold_theta(n, factor, bias=-sc.orbit_logits(bare, orc, cfg).max())
  base, fac, tau = _base('fc2x16', n, b * len(perms))
  eng, orc, _ = _compose(base, fac, tau, lat, perms, flips, chi, b, bonds=False)
  plain, _, _ = _base('fc2x16', n, b * len(perms))
  for e in (eng, plain):
    e.set_params(theta)
  base.set_shift(0.0); plain.set_shift(0.0)                # (see the head of the file)
  assert base.get_shift() == 0.0
  rows = orc.rows(cfg).reshape(-1, n)                      # op-major: row k B + c
  l_rows = plain.amplitude(np.ascontiguousarray(rows))[0].reshape(len(perms), b)      # a plain ctx returns the raw logit
  assert np.isfinite(l_rows).all()
  spread = l_rows.max(0) - l_rows.min(0)
  assert (spread > sc.FOLD_FACTORS[factor]).all(), spread
  ref, sign, r = sc.host_fold(l_rows, chi)
  ref = ref - plain.get_shift()
  if sc.FOLD_FACTORS[factor] >= 745.0:                     # terms did underflow to exactly 0 in the host fold, as they must on the GPU
    assert (np.exp(l_rows - l_rows.max(0)) == 0).any(0).all()
  assert np.isfinite(ref).all() and (r > 2.0 ** -30).all() and (sign != 0).all()
  logit, psi = eng.amplitude(cfg)
  err = np.abs(logit.astype(np.float64) - ref)
  bound = 2.0 ** -23 * np.maximum(1.0, np.abs(ref)) + 2.0 ** -40 / r
  print('%s %s factor %g: spread %.4g .. %.4g, logits %.4g .. %.4g, max |logit - ref| / bound = %.3g, min r = %.3g' % (
      lat, sector, factor, spread.min(), spread.max(), ref.min(), ref.max(), (err / bound).max(), r.min()))
  assert np.isfinite(logit).all() and np.isfinite(psi).all()
  assert (err <= bound).all()
  np.testing.assert_array_equal(np.signbit(psi), sign < 0)
  normal = np.abs(psi) >= np.finfo(np.float32).tiny        # (a psi below fp32's normal range is 0 or a denormal, with its finite logit)
  np.testing.assert_allclose(np.abs(psi[normal]), np.exp(logit[normal].astype(np.float64)), rtol=2e-6)
  assert (logit[~normal] < -87.0).all()
  # the chains' cache holds the same bits; a psi that rounds to 0 is no structural zero: such rows are taken as chains
  if lat == 'chain10' and factor > 1:
    assert (psi == 0).any() and np.isfinite(logit[psi == 0]).all()
  eng.set_configs(cfg)
  for x, y in zip(eng.amplitude(), (logit, psi)):
    np.testing.assert_array_equal(x, y)
  plain.close(); eng.close()


# ---- 5. ops that do not count

def test_zero_characters_are_left_out_of_every_fold():
  """q2 of the 8-site chain with exact zeros on the odd translations against the four even translations with the four
  characters that are left: the same terms in the same ascending order, so the same bits -- amplitudes, local energies
  and the scalar accumulators.  Not the gradient sums: the base contracts them over ITS rows (k_wgrad: K = batch_size of
  the base, 40 against 20, cut into plan_wgrad_slices(tiles, K, CUs) slices and summed four rows to an MFMA step), and
  with the rows op-major the four ops that carry weight sit at other places of that loop.  The rows of weight 0 add exact
  zeros, so the terms are the same and only their association differs (measured: 150 of 866 sums differ, by at most
  1.6e-6 relative); the sums are held to the gradient bound of tests/test_gpu_symmetrized.py against the oracle."""
  lat, n, b = 'chain8', 8, 5
  L = sc.LATTICES[lat]
  perms8, _, _ = sc.ops(lat, 'q0')
  chi8 = sc.CHI_Q2_EXACT
  assert (chi8[1::2] == 0).all() and (chi8[0::2] != 0).all()
  perms4, chi4 = perms8[0::2], chi8[0::2]
  out = []
  for perms, chi in ((perms8, chi8), (perms4, chi4)):
    base, fac, tau = _base('fc2x16', n, b * len(perms))
    eng, orc, tau = _compose(base, fac, tau, lat, perms, None, chi, b)
    cfg = sc.configs(n, b, sc.ZERO_CHI_SEED, orc)
    host = sc.configs(n, 2 * b + 3, sc.ZERO_CHI_SEED + 1)
    _check_amplitudes(eng, orc, host, tau, 'chain8 q2 n_ops=%d' % len(perms))
    eng.set_configs(cfg)
    e, mean = eng.local_energy()
    assert np.isfinite(e).all()
    eng.reset_accumulators()
    eng.accumulate(MODE)
    res = eng.get_accumulators()
    p = orc.num_params
    out.append((cfg,) + eng.amplitude(host) + eng.amplitude() + (e, res[2 * p:], res[:2 * p]))
    eng.close()
  names = ('configs', 'host logits', 'host psi', 'own logits', 'own psi', 'local energies', 'scalar accumulators')
  for name, x, y in zip(names, out[0], out[1]):
    np.testing.assert_array_equal(x, y, err_msg=name)
  acc = vo.Accumulators(p, np.float64)
  pro.energy_gradient_accumulate(acc, orc, cfg, L['bonds'], *sc.couplings(lat))
  ref = np.r_[acc.g1_total, acc.g2_total]
  r_min = orc.cancellation(cfg).min()
  bound = 4e-3 * np.abs(ref).max() + 2e-4
  for n_ops, got in ((8, out[0][-1]), (4, out[1][-1])):
    err = r_min * np.abs(got - ref).max()
    print('chain8 q2 n_ops=%d gradient sums: min r x max error %.3g (bound %.3g), min r %.3g' % (n_ops, err, bound, r_min))
    assert err <= bound
  assert r_min * np.abs(out[0][-1] - out[1][-1]).max() <= bound


def test_zero_characters_stay_out_of_the_max_shift():
  """The same two engines with the last layer scaled until, on some rows, an odd translation's logit lies more than 745
  above every even one's.  chi_k = 0 makes such an op's term vanish whatever it is, so only the shift m = max_k l_k can
  tell whether the op was skipped: were it let in, every term that counts would underflow to 0 and the row be taken for a
  structural zero.  (No oracle here: its fp64 exp has left its range too.  The bits of the four-op engine are the claim.)"""
  lat, n, b = 'chain8', 8, 5
  perms8, _, _ = sc.ops(lat, 'q0')
  chi8 = sc.CHI_Q2_EXACT
  host = sc.configs(n, 2 * b + 3, sc.ZERO_CHI_SEED + 1)
  bare = sc.fold_theta(n, sc.ZERO_CHI_FACTOR)
  l = sc.orbit_logits(bare, sc.fc_oracle(lat, 'q0', bare), host)
  gap = l[1::2].max(0) - l[0::2].max(0)
  far = gap > 1.05 * 745.0                                 # rows whose largest logit belongs to an op that does not count
  assert far.sum() >= 2, gap
  own = sc.configs(n, b, sc.ZERO_CHI_SEED, so.Symmetrized(pro.fc_factor(sc.fold_theta(n, 1.0), 16, 2), perms8, None, chi8))
  theta = sc.fold_theta(n, sc.ZERO_CHI_FACTOR, bias=-l.max())      # (the largest logit at 0: psi stays in range at the base's shift)
  out = []
  for perms, chi in ((perms8, chi8), (perms8[0::2], chi8[0::2])):
    base, fac, tau = _base('fc2x16', n, b * len(perms))
    eng, _, _ = _compose(base, fac, tau, lat, perms, None, chi, b, bonds=False)
    eng.set_params(theta)
    logit, psi = eng.amplitude(host)
    eng.set_configs(own)
    out.append((logit, psi) + eng.amplitude())
    eng.close()
  assert np.isfinite(out[1][0][far]).all() and np.isfinite(out[1][2]).all() and not np.isnan(out[1][1]).any()
  for name, x, y in zip(('host logits', 'host psi', 'own logits', 'own psi'), out[0], out[1]):
    np.testing.assert_array_equal(x, y, err_msg=name)


@pytest.mark.parametrize('sector', sc.ZERO_AMP['sectors'])
def test_zero_amplitudes_of_some_ops_of_a_row(sector):
  """An ed_vector base with exact zeros: an op whose row hits one does not count -- c_k = 0, its E_k (the base divided by
  a vanishing amplitude) is never read -- while the row's other ops carry psi_s."""
  from cgs_vmc_amd.engine import VmcEngine
  lat, n, b = 'chain8', 8, sc.ZERO_AMP['b']
  L = sc.LATTICES[lat]
  vec, top, bot = sc.zero_vector(n)
  perms, flips, chi = sc.ops(lat, sector)
  fac = pro.edvec_factor(vec, top, bot)
  base = VmcEngine(n, b * len(perms), 1, len(vec), ansatz='ed_vector', lin_tables=(top, bot))
  base.set_params(vec)
  eng, orc, tau = _compose(base, fac, None, lat, perms, flips, chi, b)
  cfg, partial = sc.zero_amp_batch(orc)
  dead = (orc.terms(cfg) == 0).sum(0)
  assert partial.any() and ((dead[partial] > 0) & (dead[partial] < len(perms))).all()      # some but not all ops on a zero
  assert (orc.psi(cfg) != 0).all() and (orc.cancellation(cfg) > 1e-3).all()
  _check_amplitudes(eng, orc, cfg, tau, 'edvec chain8 %s with zeros' % sector)
  eng.set_configs(cfg)
  _check_local_energies(eng, orc, cfg, lat, tau, 'edvec chain8 %s with zeros' % sector)
  e, mean = eng.local_energy()
  assert np.isfinite(e).all() and np.isfinite(mean)
  # c_k = 0 on the ops that do not count: the gradient sums are the oracle's (which gives such an op no weight and no O)
  eng.reset_accumulators()
  eng.accumulate(MODE)
  p = orc.num_params
  acc = vo.Accumulators(p, np.float64)
  bx, bz = sc.couplings(lat, *COUPLING_SETS[-1])           # (the set _check_local_energies left in place)
  pro.energy_gradient_accumulate(acc, orc, cfg, L['bonds'], bx, bz)
  res = eng.get_accumulators()
  assert np.isfinite(res).all()
  r_min = orc.cancellation(cfg).min()
  for got, ref, what in ((res[:p], acc.g1_total, 'g1'), (res[p:2 * p], acc.g2_total, 'g2')):
    err, bound = r_min * np.abs(got - ref).max(), 4e-3 * np.abs(ref).max() + 2e-4
    print('edvec chain8 %s with zeros %s: min r x max error %.3g (bound %.3g), min r %.3g' % (sector, what, err, bound, r_min))
    assert err <= bound
  assert (res[:p][vec == 0] == 0).all() and (res[p:2 * p][vec == 0] == 0).all()      # nothing flows into a zero entry
  # a row whose ops all hit zeros is a structural zero: refused, the chains stay
  bad = cfg.copy(); bad[3] = sc.DOMAIN_WALL
  with pytest.raises(ValueError, match='row 3 is at a structural zero'):
    eng.set_configs(bad)
  np.testing.assert_array_equal(eng.get_configs(), cfg)
  logit, psi = eng.amplitude(bad)
  assert psi[3] == 0 and np.isneginf(logit[3]) and (psi[[0, 1, 2, 4]] != 0).all() and not np.isnan(logit).any()
  eng.close()


# ---- 6. gradient sums at the new shapes

@pytest.mark.parametrize('lat,sector,b', sc.GRADIENT_CASES)
def test_gradient_sums_at_the_new_shapes(lat, sector, b):
  L = sc.LATTICES[lat]
  theta_seed, seed = sc.GRADIENT_SEEDS[(lat, sector, b)]
  eng, orc, tau = _make('fc2x16', lat, sector, b, seed=theta_seed)
  np.testing.assert_array_equal(eng.get_params(), sc.fc_theta(L['n'], theta_seed))      # (the parameters the seed table was made with)
  cfg = sc.configs(L['n'], b, seed, orc)
  r_min = orc.cancellation(cfg).min()
  assert r_min >= sc.R_MIN
  eng.set_configs(cfg)
  p = orc.num_params
  eng.reset_accumulators()
  eng.accumulate(MODE)
  acc = vo.Accumulators(p, np.float64)
  bx, bz = sc.couplings(lat)
  e_ref = pro.energy_gradient_accumulate(acc, orc, cfg, L['bonds'], bx, bz)
  res = eng.get_accumulators()

  def close(got, ref, what, atol=2e-4):
    err = r_min * np.abs(got - ref).max()
    bound = 4e-3 * np.abs(ref).max() + atol
    print('fc2x16 %s %s B=%d %s: min r x max error %.3g (bound %.3g), min r %.3g' % (lat, sector, b, what, err, bound, r_min))
    assert err <= bound, (what, err, bound)
  close(res[:p], acc.g1_total, 'g1'); close(res[p:2 * p], acc.g2_total, 'g2')
  assert r_min * abs(res[2 * p] - acc.e_total) <= tau * b * max(1.0, np.abs(e_ref).max())
  assert res[2 * p + 1] == b and res[2 * p + 4] == 1
  close(eng.get_gradient(MODE), vo.energy_gradient(acc), 'gradient', 4e-4)
  eng.close()

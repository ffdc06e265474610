"""GPU: Lanczos-step energies (vmc_energy_moments: csrc/vmc_api_measure.hip + moments.hip; LanczosStepEvaluator;
run_lanczos_evaluation) against the fp64 oracle tests/moments_oracle.py.  Families, shapes and per-row bounds are those of
tests/test_gpu_renyi.py: the 4 x 4 torus, N = 16, H = 32, B = 40 chains (no multiple of the 8- or 16-chain tiles).

Bound.  With hx, qz the couplings, D(y) = sum_b qz_b y_i y_j, v_a = hx_a r(x^a) the first-order values and
  g(x) = D(x) e(x) + sum_a v_a D(x^a) + sum_(rule 1) hx_a hx_b + sum_(rows) coef r(x^{ab}),      e(x) = D(x) + sum_a v_a,
the library takes v_a and e from the local-energy call in fp32 and adds everything else in fp64 (D, D(x^a), hx_a hx_b and
coef are sums and products of a few fp32 couplings and +-1 spins: their fp64 error goes into the summation term).
  * A ratio r = psi(row) / psi(x) is exp of the difference of two fp32 logs ln|psi|.  With eps_r the bound the family's own
    amplitude / logit parity test applies to ln|psi| of row r (tests/test_gpu_renyi.py: _family), the ratio is within
    |r| delta, delta = exp(eps_row + eps_x) - 1, of the oracle's -- as tests/test_gpu_dimer.py takes it; it enters g times
    its coefficient.
  * The fp32 v_a carries its ratio's |v_a| delta_a and one fp32 spacing of its magnitude; it enters g times |D(x^a)|.
  * The fp32 e carries the ratio errors of the values it sums, sum_a |v_a| delta_a, and one fp32 spacing of its magnitude;
    it enters g times |D(x)|.
  * The fp64 sum of T terms in a fixed order adds T 2^-53 sum |terms|.
So, per chain,
  b_e = sum_a |v_a| delta_a + spacing32(e)
  b_g = sum_rows |coef r_ab| delta_ab + sum_a (|v_a| delta_a + spacing32(v_a)) |D(x^a)| + b_e |D(x)| + T 2^-53 sum |terms|
and for the sums over the chains, with S the fp64 fold term B 2^-53 sum_c |term_c|:
  e_sum: sum_c b_e + S;  g_sum: sum_c b_g + S;  e2_sum: sum_c (2 |e| b_e + b_e^2) + S;
  eg_sum: sum_c (|e| b_g + |g| b_e + b_e b_g) + S;  g2_sum: sum_c (2 |g| b_g + b_g^2) + S.
A chain whose own amplitude vanishes has e = g = 0 on both sides.  n_rows2 and n_alive are integers: equal.
"""
import functools

import numpy as np
import pytest

from cgs_vmc_amd import _hip
from cgs_vmc_amd import lattice
from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo
from tests import moments_oracle as mo
from tests import test_gpu_renyi as tr

pytestmark = pytest.mark.gpu
N, H, B = tr.N, tr.H, tr.B
BONDS = [tuple(b) for b in tr.BONDS]
SIGNED = ('pbdg', 'fully_connected_nnb', 'ed_vector')
SUMS = ('e_sum', 'e2_sum', 'g_sum', 'eg_sum', 'g2_sum')


def _jx(ansatz):
  return 1.0 if ansatz in SIGNED else -1.0


def _key(x):
  return tuple(float(s) for s in x)


def _reference(psi, eps, cfg, bonds, j_x, j_z):
  """The oracle's e, g [B] and sums, the bounds of this file's docstring, n_rows2, n_alive and the places where the chains'
  rows start in the list."""
  cfg = np.asarray(cfg, np.float32)
  bonds = [tuple(b) for b in bonds]
  hx, qz = mo.couplings(len(bonds), j_x, j_z)
  lists = [mo.second_order_rows(x, bonds) for x in cfg]
  every = sorted({_key(x) for x in cfg} | {y for first, rows, _ in lists for _, y in first} |
                 {y for _, rows, _ in lists for _, _, _, y in rows})
  arr = np.array(every, np.float32)
  amp = dict(zip(every, np.asarray(psi(arr), np.float64)))
  tol = dict(zip(every, np.asarray(eps(arr), np.float64)))
  e_ref, g_ref, alive = mo.local_values(psi, cfg, bonds, j_x, j_z)
  diag = lambda y: sum(qz[b] * y[i] * y[j] for b, (i, j) in enumerate(bonds))
  sp32 = lambda v: float(np.spacing(np.float32(abs(v))))
  b_e, b_g = np.zeros(len(cfg)), np.zeros(len(cfg))
  starts, n2 = [], 0
  for c, (x, (first, rows, selfs)) in enumerate(zip(cfg, lists)):
    starts.append(n2)
    n2 += len(rows)
    x = _key(x)
    if amp[x] == 0:
      assert not alive[c] and e_ref[c] == 0 and g_ref[c] == 0
      continue
    delta = lambda y: np.expm1(tol[y] + tol[x]) if amp[y] != 0 else 0.0
    d_x = diag(x)
    terms, be, bg = [abs(d_x * e_ref[c])], 0.0, 0.0
    for a, xa in first:
      v = hx[a] * amp[xa] / amp[x]
      dv = abs(v) * delta(xa)
      be += dv
      bg += (dv + sp32(v)) * abs(diag(xa))
      terms.append(abs(v * diag(xa)))
    be += sp32(e_ref[c])
    bg += be * abs(d_x)
    for a, b, mult, y in rows:
      t = abs(mult * hx[a] * hx[b] * amp[y] / amp[x])
      bg += t * delta(y)
      terms.append(t)
    terms += [abs(hx[a] * hx[b]) for a, b in selfs]
    b_e[c] = be
    b_g[c] = bg + len(terms) * 2.0 ** -53 * sum(terms)
  fold = lambda t: len(cfg) * 2.0 ** -53 * np.abs(t).sum()
  ae, ag = np.abs(e_ref), np.abs(g_ref)
  sums = {'e_sum': e_ref.sum(), 'e2_sum': (e_ref ** 2).sum(), 'g_sum': g_ref.sum(), 'eg_sum': (e_ref * g_ref).sum(),
          'g2_sum': (g_ref ** 2).sum()}
  bounds = {'e_sum': b_e.sum() + fold(e_ref), 'g_sum': b_g.sum() + fold(g_ref),
            'e2_sum': (2 * ae * b_e + b_e ** 2).sum() + fold(e_ref ** 2),
            'eg_sum': (ae * b_g + ag * b_e + b_e * b_g).sum() + fold(e_ref * g_ref),
            'g2_sum': (2 * ag * b_g + b_g ** 2).sum() + fold(g_ref ** 2)}
  return {'e': e_ref, 'g': g_ref, 'b_e': b_e, 'b_g': b_g, 'sums': sums, 'bounds': bounds, 'n_rows2': n2,
          'n_alive': int(alive.sum()), 'alive': alive, 'starts': starts + [n2]}


@functools.lru_cache(maxsize=None)
def _family_reference(ansatz, cfg_seed=2):
  theta, psi, eps = tr._family(ansatz)
  cfg = tr._cfg(cfg_seed)
  return theta, cfg, _reference(psi, eps, cfg, BONDS, _jx(ansatz), 1.0)


def _check(tag, got, ref):
  """h2_loc and the six sums against the oracle; e_loc within its bound too.  Prints the worst error over bound first."""
  err_g, err_e = np.abs(got['h2_loc'] - ref['g']), np.abs(got['e_loc'] - ref['e'])
  with np.errstate(divide='ignore', invalid='ignore'):
    rel_g = np.where(ref['b_g'] > 0, err_g / ref['b_g'], np.where(err_g == 0, 0.0, np.inf))
    rel_e = np.where(ref['b_e'] > 0, err_e / ref['b_e'], np.where(err_e == 0, 0.0, np.inf))
  k = int(np.argmax(rel_g))
  line = '%s: h2_loc worst error / bound %.3g (chain %d: error %.3g, bound %.3g, value %.9g); e_loc %.3g;' % (
      tag, rel_g[k], k, err_g[k], ref['b_g'][k], ref['g'][k], rel_e.max())
  for name in SUMS:
    line += ' %s %.3g' % (name, abs(got[name] - ref['sums'][name]) / ref['bounds'][name])
  print(line)
  assert np.isfinite(got['h2_loc']).all() and np.isfinite(got['e_loc']).all(), tag
  assert all(np.isfinite(got[name]) for name in SUMS), tag
  assert got['n_rows2'] == ref['n_rows2'] and got['n_alive'] == ref['n_alive'], (tag, got['n_rows2'], ref['n_rows2'])
  assert (err_g <= ref['b_g']).all(), (tag, k, err_g[k], ref['b_g'][k])
  assert (err_e <= ref['b_e']).all(), (tag, int(np.argmax(rel_e)), rel_e.max())
  for name in SUMS:
    assert abs(got[name] - ref['sums'][name]) <= ref['bounds'][name], (tag, name, got[name], ref['sums'][name], ref['bounds'][name])


def _same(a, b):
  assert set(a) == set(b)
  for k in a:
    np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _ascending_sum(values):
  s = np.float64(0.0)
  for v in np.asarray(values, np.float64):
    s = s + v
  return float(s)


@pytest.mark.parametrize('ansatz', tr.FAMILIES)
def test_local_values_match_the_fp64_oracle(ansatz):
  theta, cfg, ref = _family_reference(ansatz)
  assert (cfg.sum(1) == 0).all()
  eng = tr._engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(BONDS, _jx(ansatz), 1.0)
  got = eng.energy_moments(per_chain=True)
  _check(ansatz, got, ref)
  # the local energies are local_energy()'s, bit for bit, and e_sum is their ascending fp64 sum
  eloc, _ = eng.local_energy()
  alive = ref['alive']
  np.testing.assert_array_equal(got['e_loc'][alive], eloc[alive].astype(np.float64))
  assert got['e_sum'] == _ascending_sum(eloc[alive])
  assert got['g_sum'] == _ascending_sum(got['h2_loc'][alive])
  assert got['e2_sum'] == _ascending_sum(got['e_loc'][alive] * got['e_loc'][alive])
  assert got['eg_sum'] == _ascending_sum(got['e_loc'][alive] * got['h2_loc'][alive])
  assert got['g2_sum'] == _ascending_sum(got['h2_loc'][alive] * got['h2_loc'][alive])
  if ansatz == 'ed_vector':
    assert 0 < ref['n_alive'] < B                        # chains whose own amplitude vanishes: 0, never NaN, not alive
    assert (got['e_loc'][~alive] == 0).all() and (got['h2_loc'][~alive] == 0).all()
  else:
    assert ref['n_alive'] == B
  assert got['n_rows2'] > 64 * B                         # every chain's rows go round its 64 lanes more than once
  # without the per-chain arrays: the same sums
  plain = eng.energy_moments()
  assert set(plain) == set(got) - {'e_loc', 'h2_loc'}
  _same(plain, {k: got[k] for k in plain})
  # the supervisor's parameter set measures through the same entry
  eng.set_params(theta, _hip.VMC_OMEGA)
  _same(eng.energy_moments(which=_hip.VMC_OMEGA, per_chain=True), got)
  eng.close()


@functools.lru_cache(maxsize=None)
def _torus_ground_state():
  return eo.vector_from_ed(N, tr.BONDS, 1.0, 1.0)


def test_an_eigenstate_gives_the_energy_and_its_square_on_any_chains():
  """The 4 x 4 ground state in ed_vector: e(x) = E0 and g(x) = E0^2 on every chain, whatever the chains; the evaluator's
  algebra sees a degenerate overlap matrix."""
  from cgs_vmc_amd import evaluation
  e0, vec64, top, bot = _torus_ground_state()
  vec = vec64.astype(np.float32)
  psi = lambda c: eo.amplitude(vec.astype(np.float64), c, top, bot)
  cfg = tr._cfg(4)
  ref = _reference(psi, tr._edvec_eps(vec, top, bot), cfg, BONDS, 1.0, 1.0)
  eng = tr._engine('ed_vector')
  eng.set_params(vec); eng.set_configs(cfg); eng.set_bonds(BONDS, 1.0, 1.0)
  got = eng.energy_moments(per_chain=True)
  _check('4 x 4 ground state', got, ref)
  assert got['n_alive'] == B
  # the fp32 vector is an eigenvector to about eps32: the oracle's own values sit that close to E0 and E0^2
  slack_e, slack_g = np.abs(ref['e'] - e0).max(), np.abs(ref['g'] - e0 * e0).max()
  print('  E0 %.9f: max |e - E0| %.3g (oracle %.3g), max |g - E0^2| %.3g (oracle %.3g)' % (
      e0, np.abs(got['e_loc'] - e0).max(), slack_e, np.abs(got['h2_loc'] - e0 * e0).max(), slack_g))
  assert slack_e < 1e-4 and slack_g < 1e-3
  assert (np.abs(got['e_loc'] - e0) <= ref['b_e'] + slack_e).all()
  assert (np.abs(got['h2_loc'] - e0 * e0) <= ref['b_g'] + slack_g).all()
  out = evaluation.lanczos_step([got[k] for k in SUMS] + [got['n_alive']])
  var_bound = (ref['bounds']['e2_sum'] + 2 * abs(e0) * ref['bounds']['e_sum']) / B + 2 * abs(e0) * slack_e + slack_e ** 2
  print('  variance %.3g (bound %.3g), lanczos_energy - energy %.3g' % (out['variance'], var_bound, out['lanczos_energy'] - out['energy']))
  assert abs(out['variance']) <= var_bound
  assert out['lanczos_energy'] == out['energy'] and out['alpha'] == 0.0 and out['extrapolated_energy'] == out['energy']
  assert all(np.isfinite(out[k]) for k in evaluation.LANCZOS_QUANTITIES)
  eng.close()


# ---- the list rules

TORUS28 = [tuple(b) for b in vo.torus_bonds(2, 8)]                 # raw: the 2-wide direction names every bond twice
J1J2 = [tuple(b) for b in vo.torus_bonds(4, 4, next_nearest=True)]
DESCENDING = [(max(b), min(b)) for b in BONDS][::-1]               # sites (j, i) with j > i, the list back to front
BOND_SETS = {
    'torus 2 x 8, twin bonds': (TORUS28, lambda s: s, 1.0),
    'J1-J2 4 x 4': (J1J2, lambda s: np.where(np.arange(64) < 32, s, 0.6 * s).astype(np.float32), 1.0),
    'descending sites': (DESCENDING, lambda s: s, 1.0),
}
assert len(set(map(frozenset, TORUS28))) < len(TORUS28) and len(J1J2) == 64


@pytest.mark.parametrize('ansatz', ['fully_connected', 'pbdg'])
@pytest.mark.parametrize('name', list(BOND_SETS))
def test_list_rules(name, ansatz):
  bonds, jx_of, jz = BOND_SETS[name]
  jx = jx_of(_jx(ansatz))
  theta, psi, eps = tr._family(ansatz)
  cfg = tr._cfg(5)
  ref = _reference(psi, eps, cfg, bonds, jx, jz)
  eng = tr._engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg)
  eng.set_bonds(bonds, jx if np.ndim(jx) else float(jx), jz)
  got = eng.energy_moments(per_chain=True)
  _check('%s, %s' % (name, ansatz), got, ref)
  lists = [mo.second_order_rows(x, bonds) for x in cfg]
  if name.startswith('torus 2 x 8'):
    assert any(a != b for _, _, selfs in lists for a, b in selfs)                       # rule 1 through a twin bond
  assert any(m == 2.0 for _, rows, _ in lists for _, _, m, _ in rows)                   # rule 2
  assert any(m == 1.0 for _, rows, _ in lists for _, _, m, _ in rows)                   # rule 3
  eng.close()


# ---- passes

@pytest.mark.parametrize('ansatz', ['fully_connected', 'ed_vector'])
def test_every_pass_size_gives_the_same_bits(ansatz):
  theta, cfg, ref = _family_reference(ansatz)
  eng = tr._engine(ansatz)
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(BONDS, _jx(ansatz), 1.0)
  whole = eng.energy_moments(per_chain=True)
  _check(ansatz + ' (one pass)', whole, ref)
  starts = np.array(ref['starts'])
  ends7 = np.arange(7, ref['n_rows2'], 7)
  assert (~np.isin(ends7, starts)).any()                 # passes of 7 rows end inside chains' rows
  assert ref['n_rows2'] > 1000                           # passes of 1000 rows: more than one
  for per in (1, 7, 64, 1000):
    _same(eng.energy_moments(rows_per_pass=per, per_chain=True), whole)
  # the row buffers are shared with the siblings: nothing of theirs leaks into a later call
  eng.dimer_correlations(BONDS[:6], [(0, 1), (2, 5), (3, 3)])
  _same(eng.energy_moments(rows_per_pass=7, per_chain=True), whole)
  _same(eng.energy_moments(per_chain=True), whole)
  eng.close()


def test_h_squared_is_the_sum_of_all_dimer_pairs():
  """j_x = j_z = 1: H = sum_a S_a . S_b, so g_sum is the sum of dimer_correlations over all 32^2 ordered pairs of bonds
  and e_sum the sum of its bond sums, within the two measurements' bounds (tests/test_gpu_dimer.py builds the other)."""
  from tests import test_gpu_dimer as td
  theta, psi, eps = tr._family('fully_connected')
  cfg = tr._cfg(2)
  ref = _reference(psi, eps, cfg, BONDS, 1.0, 1.0)
  pairs = lattice.all_bond_pairs(len(BONDS))
  assert len(pairs) == 1024
  _, _, bond_bound, dd_bound = td._reference(psi, eps, cfg, BONDS, [tuple(p) for p in pairs])
  eng = tr._engine('fully_connected')
  eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(BONDS, 1.0, 1.0)
  got = eng.energy_moments()
  bond_sum, dd_sum = eng.dimer_correlations(BONDS)
  err_g, err_e = abs(got['g_sum'] - dd_sum.sum()), abs(got['e_sum'] - bond_sum.sum())
  print('g_sum %.9g vs dimers %.9g: error %.3g, bound %.3g; e_sum error %.3g, bound %.3g' % (
      got['g_sum'], dd_sum.sum(), err_g, ref['bounds']['g_sum'] + dd_bound.sum(), err_e, ref['bounds']['e_sum'] + bond_bound.sum()))
  assert err_g <= ref['bounds']['g_sum'] + dd_bound.sum()
  assert err_e <= ref['bounds']['e_sum'] + bond_bound.sum()
  eng.close()


def test_a_measurement_moves_nothing_else():
  theta, _, _ = tr._family('fully_connected')

  def prepared():
    eng = tr._engine()
    eng.set_params(theta); eng.set_configs(tr._cfg(6)); eng.set_bonds(BONDS, -1.0, 1.0)
    eng.mc_steps(3 * N)
    eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.mc_steps(N)                                      # straight from the sampler's caches into a measurement
    return eng
  eng, twin = prepared(), prepared()
  path, shifts = eng.kernel_path(), (eng.get_shift(0), eng.get_shift(1))
  first = eng.energy_moments(per_chain=True)
  _same(eng.energy_moments(rows_per_pass=50, per_chain=True), first)
  np.testing.assert_array_equal(eng.get_configs(), twin.get_configs())
  assert eng.step_counter == twin.step_counter
  np.testing.assert_array_equal(eng.get_accumulators(), twin.get_accumulators())
  assert eng.kernel_path() == path and (eng.get_shift(0), eng.get_shift(1)) == shifts
  for x, y in zip(eng.local_energy_terms(), twin.local_energy_terms()):      # the Hamiltonian's bond set answers as before
    np.testing.assert_array_equal(x, y)
  twin.local_energy()                                    # the one exception: what a local-energy call leaves behind
  eng.energy_moments()
  assert eng.last_connected_rows() == twin.last_connected_rows() > 0
  # caches that were not valid before are not vouched for after: fresh chains, a measurement on one side only
  for e in (eng, twin):
    e.mc_steps(N)
  eng.energy_moments(rows_per_pass=33)
  np.testing.assert_array_equal(eng.local_energy()[0], twin.local_energy()[0])
  for e in (eng, twin):
    e.mc_steps(N)
  np.testing.assert_array_equal(eng.get_configs(), twin.get_configs())
  eng.close(); twin.close()
  # two training epochs with and without a measurement between them: the same parameters
  params = []
  for measure in (False, True):
    eng = tr._engine(b=64, seed=77)
    eng.set_params(theta); eng.set_configs(tr._cfg(7, b=64)); eng.set_bonds(BONDS, -1.0, 1.0)
    for epoch in range(2):
      eng.epoch_energy_gradient(2 * N, 3, N, 1e10)
      eng.apply_adam(_hip.VMC_MODE_ENERGY_GRADIENT, 1e-2)
      if measure and epoch == 0:
        eng.energy_moments(rows_per_pass=100)
    params.append((eng.get_params(), eng.get_configs(), eng.step_counter))
    eng.close()
  for x, y in zip(*params):
    np.testing.assert_array_equal(x, y)


# ---- the moments end to end

N12 = 12


def _random_vector_directory(path):
  """A checkpoint directory (tools/make_ed_vector.py's) of the 12-site ring whose vector is a fixed positive random one;
  -> (the vector over the Sz = 0 basis, fp32 values in fp64, the dense Hamiltonian at j_x = -1, j_z = 1)."""
  from tools import make_ed_vector as mk
  mk.main([path, '--lattice', 'chain', '--size', str(N12)])
  basis, hmat = mo.dense_h(N12, [tuple(b) for b in lattice.chain_bonds(N12)], -1.0, 1.0)
  assert len(basis) == 924
  state = np.random.default_rng(2026).uniform(0.5, 1.5, len(basis)).astype(np.float32)
  top, bot, length = eo.lin_tables(N12)
  vec = np.zeros(length, np.float32)
  vec[eo.index(basis, top, bot)] = state
  np.savetxt(path + '/ed_vector.txt', vec, fmt='%.9g')
  np.savez(path + '/model_prior_0_epochs.npz', **{'full_vector/ed_vector': vec})
  return state.astype(np.float64), hmat


def test_sampled_moments_and_the_lanczos_step_against_dense_numpy(monkeypatch, tmp_path):
  """A fixed positive random vector on the 12-site ring (924 states, j_x = -1), sampled: 1,024 chains, 16 samples, 2 sweeps
  apart, 50 sweeps of equilibration, through LanczosStepEvaluator (the driver's evaluate); then the driver itself."""
  from cgs_vmc_amd import evaluation, run_lanczos_evaluation as rl, session, wavefunctions
  monkeypatch.setenv('CGS_VMC_SEED', '20261019')
  monkeypatch.setenv('CGS_VMC_CONFIG_SEED', '5')
  d, out_dir = str(tmp_path / 'ring'), str(tmp_path / 'out')
  state, hmat = _random_vector_directory(d)
  hn, e1, alpha, var1 = mo.exact_moments(hmat, state)
  e0 = np.linalg.eigvalsh(hmat)[0]
  exact = {'h1': hn[0], 'h2': hn[1], 'h3': hn[2], 'h4': hn[3], 'h2_check': hn[1], 'energy': hn[0],
           'variance': hn[1] - hn[0] ** 2, 'lanczos_energy': e1, 'alpha': alpha, 'lanczos_variance': var1}
  args = ['--checkpoint_dir', d, '--j_x', '-1.0', '--hparams',
          'batch_size=1024,num_evaluation_samples=16,num_monte_carlo_sweeps=2,num_equilibration_sweeps=50']
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  _, _, out = rl.evaluate(rl.cli_common.parser_from_table(rl.__doc__, rl.FLAG_TABLE).parse_args(args))
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  for k in exact:
    print('%-16s %.9g +- %.3g (exact %.9g: %.2f errors)' % (k, out[k], out[k + '_err'], exact[k],
                                                           abs(out[k] - exact[k]) / out[k + '_err']))
  print('extrapolated     %.9g +- %.3g, E0 %.9g, n_rows2 %d' % (out['extrapolated_energy'], out['extrapolated_energy_err'], e0,
                                                              out['n_rows2']))
  assert out['samples'].shape == (16, 6) and (out['samples'][:, 5] == 1024).all() and out['n_rows2'] > 0
  for k in exact:
    assert out[k + '_err'] > 0 and abs(out[k] - exact[k]) <= 5 * out[k + '_err'], k
  assert out['lanczos_energy'] < out['energy'] - 5 * max(out['lanczos_energy_err'], out['energy_err'])
  assert out['lanczos_energy'] >= e0 - 3 * out['lanczos_energy_err']
  assert np.isfinite(out['extrapolated_energy']) and out['extrapolated_energy_err'] > 0
  # the driver on the same directory: the same chains, the same numbers
  result, written = rl.main(args + ['--output_dir', out_dir])
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  assert written == [out_dir + '/lanczos.txt']
  back = rl.read_lanczos(written[0])
  assert list(back) == list(evaluation.LANCZOS_QUANTITIES)
  for k in evaluation.LANCZOS_QUANTITIES:
    np.testing.assert_allclose(back[k], (out[k], out[k + '_err']), rtol=1e-9, err_msg=k)
    assert result[k] == back[k][0]


# ---- refusals

def _raw(eng, which=0, rows_per_pass=0):
  """The C entry itself: the return code, the ctx's message, and that a refused call writes nothing."""
  fn = eng._lib.vmc_energy_moments
  dp = fn.argtypes[3]
  sums, e, g = np.full(6, np.nan), np.full(eng.batch_size, np.nan), np.full(eng.batch_size, np.nan)
  n2 = np.array([-7], np.int64)
  rc = fn(eng._ctx, which, rows_per_pass, sums.ctypes.data_as(dp), e.ctypes.data_as(dp), g.ctypes.data_as(dp),
          n2.ctypes.data_as(fn.argtypes[6]))
  if rc != _hip.VMC_OK:
    assert np.isnan(sums).all() and np.isnan(e).all() and np.isnan(g).all() and n2[0] == -7
  return rc, eng._lib.vmc_last_error(eng._ctx).decode()


def test_refusals():
  from cgs_vmc_amd.engine import VmcEngine
  theta, cfg, ref = _family_reference('fully_connected')
  eng = tr._engine()
  eng.set_params(theta); eng.set_configs(cfg)
  rc, msg = _raw(eng)
  assert rc == _hip.VMC_ERR_STATE and 'vmc_set_bonds' in msg
  with pytest.raises(_hip.HipLibraryError, match='bonds not set'):
    eng.energy_moments()
  eng.set_bonds(BONDS, -1.0, 1.0)
  assert _raw(eng, which=2)[0] == _hip.VMC_ERR_INVALID
  rc, msg = _raw(eng, rows_per_pass=-1)
  assert rc == _hip.VMC_ERR_INVALID and 'rows_per_pass' in msg
  with pytest.raises(ValueError):
    eng.energy_moments(which=2)
  with pytest.raises(ValueError):
    eng.energy_moments(rows_per_pass=-1)
  assert _raw(eng)[0] == _hip.VMC_OK
  _check('after the refusals', eng.energy_moments(per_chain=True), ref)
  eng.close()
  tanh = VmcEngine(N, B, 2, H, output_activation='tanh', seed=2024)
  tanh.set_params(theta); tanh.set_configs(cfg); tanh.set_bonds(BONDS, -1.0, 1.0)
  assert _raw(tanh)[0] == _hip.VMC_ERR_UNSUPPORTED
  with pytest.raises(NotImplementedError, match='exp output'):
    tanh.energy_moments()
  tanh.close()
  spec = dict(ansatz='fully_connected', num_layers=1, layer_size=H, nonlinearity='relu', output_activation='exp')
  prod = VmcEngine(N, B, 0, 0, ansatz='prod', children=[spec, dict(spec, ansatz='rbm')], seed=2024)
  assert _raw(prod)[0] == _hip.VMC_ERR_UNSUPPORTED
  with pytest.raises(NotImplementedError, match='product ctx'):
    prod.energy_moments()
  assert _raw(prod.children[0])[0] == _hip.VMC_ERR_STATE
  with pytest.raises(_hip.ComposedFactorError):
    prod.children[0].energy_moments()
  prod.close()

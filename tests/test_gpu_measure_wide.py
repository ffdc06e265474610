"""GPU: the three measurements (vmc_pair_correlations, vmc_renyi2_swap, vmc_dimer_correlations) beyond 64 sites and off the
narrow row kernel.  tests/test_gpu_corr.py, test_gpu_renyi.py and test_gpu_dimer.py run at N <= 24 and H = 32, where the
row builders' site loops (q = lane; q < N; q += 64) make one trip and every forward takes the narrow fused kernel; here
N = 100 (two trips, the second partial), 66 (two lanes in the second trip) and 128 (two full trips), B = 26 (even for the
replica pairs, no multiple of 8 or 16), and the forwards of kernel paths 0 (H = 48: not its own padded width), 1 (257
units: launch_tail_lds), 2 (513 units: wide_forward), 3 (fused convolution, 12 x 12) and 6 (general convolution).

Two checks per case.
(1) The fp64 oracle, with the bound formulas of tests/test_gpu_renyi.py / test_gpu_dimer.py / test_gpu_corr.py and the
    per-row eps of the family's own amplitude test at that width (the constants in _family, each beside its source).
(2) The library's own rows: the exchanged / swapped configurations built on the host in the row kernels' layout (row =
    item * B + chain, the chain's own configuration where nothing is exchanged), their ln|psi| from eng.amplitude(rows) --
    the same rows_forward_device call on the same rows -- folded on the host in the fold kernels' order and arithmetic in
    fp64.  Agreement within (B 2^-53 + 2^-51) sum |terms|: the fold's own rounding plus one ulp for the device's double
    exp.  This pins row offsets, the match and antiparallel bits and the row contents independently of fp32 forward error.
    (The spin correlations take their rows from the local-energy kernels, which hand back fp32 ratios: their fold is held
    to the host sum of local_energy_terms' rows, as in tests/test_gpu_corr.py.)
Bit identity across regions_per_pass / pairs_per_pass in (0, 1, 7) and across a second call is asserted once per N."""
import numpy as np
import pytest

from cgs_vmc_amd import lattice
from oracle import vmc_oracle as vo
from tests import corr_oracle as co
from tests import dimer_oracle as do
from tests import renyi_oracle as ro
from tests import test_gpu_dimer as td
from tests import test_gpu_renyi as tr

pytestmark = pytest.mark.gpu
B = 26
HALF = B // 2
CONV_GEOM = (8, 3, 12, 12)                 # 8 filters, 3 x 3 taps, 12 x 12 sites

CASES = [
    # id, ansatz, N, H (filters), layers, expected kernel_path(), force the general convolution path, pass splits too
    ('fc-N100-H48-path0', 'fully_connected', 100, 48, 2, 0, False, True),
    ('fc-N100-H257-path1', 'fully_connected', 100, 257, 2, 1, False, False),     # the smallest width of the LDS-operand kernels
    ('fc-N100-H513-path2', 'fully_connected', 100, 513, 2, 2, False, False),     # the smallest width of the general dense path
    ('rbm-N100-H48-path0', 'rbm', 100, 48, 1, 0, False, False),
    ('rbm-N100-H257-path1', 'rbm', 100, 257, 1, 1, False, False),
    ('conv-12x12-F8-path3', 'conv_2d', 144, 8, 2, 3, False, False),
    ('conv-12x12-F8-path6', 'conv_2d', 144, 8, 2, 6, True, False),
    ('fc-N66-H48-path0', 'fully_connected', 66, 48, 2, 0, False, True),
    ('fc-N128-H48-path0', 'fully_connected', 128, 48, 2, 0, False, True),
]
IDS = [c[0] for c in CASES]


def _lattice_bonds(n):
  if n == 100:
    return [tuple(b) for b in vo.torus_bonds(10, 10)]
  if n == 144:
    return [tuple(b) for b in vo.torus_bonds(12, 12)]
  return [tuple(b) for b in vo.chain_bonds(n)]


def _family(ansatz, n, h, L, seed=0):
  """(theta fp32, psi(configs) fp64 oracle, eps(configs) -> the per-row bound on ln|psi| of the family's parity test)."""
  rng = np.random.default_rng(seed)
  if ansatz == 'fully_connected':
    theta = vo.init_params(n, h, L, rng)
    # tests/test_gpu_engine.py (test_amplitude_matches_oracle) for <= 256 units, tests/test_gpu_wide.py (_check_forward_and_sampler:
    # _close(..., 2e-5)) for 257 .. 512 and beyond: |dlogit| <= 2e-5 max(1, |logit|)
    eps = lambda c: 2e-5 * np.maximum(1.0, np.abs(vo.fc_logit(theta, c, h, L, dtype=np.float64)))
    return theta, (lambda c: vo.fc_psi(theta, c, h, L, dtype=np.float64)), eps
  if ansatz == 'rbm':
    theta = vo.rbm_init_params(n, h, L, rng)
    # tests/test_gpu_rbm.py (test_rbm_amplitude_and_local_energy, shapes up to 640 units): |dlogit| <= 2e-5 max(1, |logit|)
    eps = lambda c: 2e-5 * np.maximum(1.0, np.abs(vo.rbm_logit(theta, c, h, L, dtype=np.float64)))
    return theta, (lambda c: vo.rbm_psi(theta, c, h, L, dtype=np.float64)), eps
  theta = vo.conv_init_params('conv_2d', CONV_GEOM, L, rng)
  theta = theta + (0.03 * rng.standard_normal(theta.size)).astype(np.float32)      # tests/test_gpu_conv.py::_make's noise
  # tests/test_gpu_conv.py (_logits_close; tests/test_gpu_conv_general.py applies the same on the general path):
  # |dlogit| <= 1e-6 sum |entries of the last map| + 2e-5
  eps = lambda c: 1e-6 * vo.conv_forward(theta, c, 'conv_2d', CONV_GEOM, L, 'relu', np.float64, return_tape='scale')[1] + 2e-5
  return theta, (lambda c: vo.ANSATZ['conv_2d'][0](theta, c, CONV_GEOM, L, dtype=np.float64)), eps


def _engine(ansatz, n, h, L, general, monkeypatch):
  from cgs_vmc_amd.engine import VmcEngine
  if ansatz == 'conv_2d':
    if general:
      monkeypatch.setenv('CGS_VMC_CONV_GENERAL', '1')
    else:
      monkeypatch.delenv('CGS_VMC_CONV_GENERAL', raising=False)
    return VmcEngine(n, B, L, h, ansatz=ansatz, kernel_size=3, size_x=12, size_y=12, seed=2024)
  return VmcEngine(n, B, L, h, ansatz=ansatz, seed=2024)


def _regions(n):
  """The blocks l = 1 .. N / 2, a region across the 64-site boundary, one wholly beyond it, the empty set, the full set."""
  return lattice.block_regions(n) + [sorted({3, 63, 64, 65, n - 1}), [64, 65], [], list(range(n))]


def _bonds(n):
  """The lattice's own bonds, the three across / beyond the 64-site boundary and a pair of sites that is no bond."""
  own = _lattice_bonds(n)
  extra = [(63, 64), (64, 65), (2, n - 1), (5, 40)]
  out = own + [b for b in extra if b not in own and (b[1], b[0]) not in own]
  assert (5, 40) in out and len(set(out)) == len(out)
  return out


def _bond_pairs(bonds, n):
  """tests/test_gpu_dimer.py::_pair_list's choice -- a disjoint partner, one sharing a site, a == a, both orders -- for 15
  first bonds: about 70 pairs, so that the fold's second 64-thread block has work.  Among the first bonds: the boundary bonds."""
  index = {b: k for k, b in enumerate(bonds)}
  first = [0, 5, 17, len(bonds) // 2, len(bonds) - 1]                   # (the last one: the pair of sites that is no bond)
  first += [index[b] if b in index else index[(b[1], b[0])] for b in ((63, 64), (64, 65), (2, n - 1))]
  first = list(dict.fromkeys(first))
  k = 7
  while len(first) < 15:
    if k not in first:
      first.append(k)
    k = (k + 11) % len(bonds)
  pairs = []
  for a in first:
    sa = set(bonds[a])
    disjoint = next(b for b in range(len(bonds) - 1, -1, -1) if not sa & set(bonds[b]))       # (from the far end: beyond site 63)
    sharing = next(b for b in range(len(bonds)) if b != a and len(sa & set(bonds[b])) == 1)
    for b in (disjoint, sharing):
      pairs += [(a, b), (b, a)]
    pairs.append((a, a))
  pairs = list(dict.fromkeys(pairs))                                    # (a partner may be another first bond)
  assert 64 < len(pairs) <= 75
  return pairs


def _site_pairs(n):
  """About 300 of all pairs (fixed seed) plus the four boundary pairs: more than the 256-bond prefetch groups."""
  every = lattice.all_pairs(n)
  pick = every[np.sort(np.random.default_rng(21).permutation(len(every))[:296])]
  boundary = np.array([(63, 64), (64, 65), (2, n - 1), (5, 40)], np.int32)
  keep = [p for p in pick.tolist() if tuple(p) not in {tuple(x) for x in boundary.tolist()}]
  return np.array(boundary.tolist() + keep, np.int32)


def _ascending(terms):
  """[items][chains] -> [items]: the chains added in ascending order in fp64, as the fold kernels add them."""
  out = np.zeros(len(terms))
  for k, row in enumerate(terms):
    s = 0.0
    for t in row:
      s += t
    out[k] = s
  return out


def _assert_rows_alive(psi, rows, tag):
  """CPU precondition of both checks: the oracle's amplitudes of every row are finite and non-zero in fp64."""
  with np.errstate(over='ignore'):
    a = np.concatenate([np.asarray(psi(rows[k:k + 2048]), np.float64) for k in range(0, len(rows), 2048)])
  assert np.isfinite(a).all() and (a != 0).all(), tag


def _own_rows_check(tag, got, host, terms_abs):
  bound = (B * 2.0 ** -53 + 2.0 ** -51) * terms_abs
  err = np.abs(got - host)
  with np.errstate(divide='ignore', invalid='ignore'):
    rel = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
  k = int(np.argmax(rel))
  print('%s vs the host fold of the library\'s own rows: worst |diff| / bound %.3g (entry %d: diff %.3g, bound %.3g)' % (tag, rel[k], k, err[k], bound[k]))
  assert (err <= bound).all(), (tag, k, got[k], host[k], bound[k])


def _swap_rows(cfg, masks):
  """k_swap_rows on the host: rows [n_regions * B][N], row = region * B + chain; (rows, match [n_regions][B / 2])."""
  x, y = cfg[:HALF], cfg[HALF:]
  rows = np.tile(cfg, (len(masks), 1)).reshape(len(masks), B, -1)
  match = np.zeros((len(masks), HALF), bool)
  for k, m in enumerate(masks):
    match[k] = x[:, m].astype(np.int64).sum(1) == y[:, m].astype(np.int64).sum(1)
    hit = np.flatnonzero(match[k])
    sel = np.ix_(hit, np.flatnonzero(m))
    rows[k, :HALF][sel] = y[sel]
    rows[k, HALF:][sel] = x[sel]
  return rows.reshape(len(masks) * B, -1), match


def _check_renyi(tag, eng, psi, eps, cfg, n, splits):
  regions = _regions(n)
  masks = ro.masks(regions, n)
  rows, match = _swap_rows(cfg, masks)
  _assert_rows_alive(psi, rows, tag + ' swapped rows')
  swap, count = eng.renyi2_swap(regions)
  # (1) the oracle
  ref_swap, ref_count, bound = tr._reference(psi, eps, cfg, masks)
  np.testing.assert_array_equal(count, ref_count)
  np.testing.assert_array_equal(count, match.sum(1))
  assert np.isfinite(swap).all()
  tr._check(tag + ' swap_sum', swap, ref_swap, bound)
  blocks = count[:n // 2]
  assert (blocks > 0).sum() >= n // 8 and blocks.max() < HALF           # the blocks see matching and non-matching pairs
  assert 0 < count[n // 2] and 0 < count[n // 2 + 1]                    # ... and the two regions at the 64-site boundary match somewhere
  assert count[-1] == HALF and count[-2] == HALF
  # (2) the library's own rows, folded as k_swap_fold folds them
  own = eng.amplitude()[0].astype(np.float64)
  rl = eng.amplitude(rows)[0].astype(np.float64).reshape(len(masks), B)
  terms = np.where(match, np.exp((rl[:, :HALF] + rl[:, HALF:]) - (own[:HALF] + own[HALF:])[None, :]), 0.0)
  _own_rows_check(tag + ' swap_sum', swap, _ascending(terms), np.abs(terms).sum(1))
  if splits:
    for per in (0, 1, 7):
      for _ in range(2):
        s, m = eng.renyi2_swap(regions, regions_per_pass=per)
        np.testing.assert_array_equal(s, swap, err_msg='regions_per_pass=%d' % per)
        np.testing.assert_array_equal(m, count, err_msg='regions_per_pass=%d' % per)


def _check_dimer(tag, eng, psi, eps, cfg, n, splits):
  bonds = _bonds(n)
  pairs = _bond_pairs(bonds, n)
  # k_dimer_rows1 / k_dimer_rows2 on the host, with the oracle's row builders
  own_psi = np.asarray(psi(cfg), np.float64)
  rows1 = np.empty((len(bonds), B, n), np.float32)
  anti1 = np.zeros((len(bonds), B), bool)
  for a, bond in enumerate(bonds):
    anti1[a] = cfg[:, bond[0]] != cfg[:, bond[1]]
    rows1[a] = np.where(anti1[a][:, None], do.exchanged(cfg, *bond), cfg)
  rows2 = np.empty((len(pairs), B, n), np.float32)
  anti2 = np.zeros((len(pairs), B), bool)
  spins2 = []
  for p, (a, b) in enumerate(pairs):
    xp = do.exchanged(cfg, *bonds[a])
    k, l = bonds[b]
    anti2[p] = anti1[a] & (xp[:, k] != xp[:, l])
    rows2[p] = np.where(anti2[p][:, None], do.exchanged(xp, k, l), cfg)
    spins2.append((xp[:, k].astype(np.float64) * xp[:, l]))
  assert anti2.any(1).sum() > len(pairs) // 2 and (~anti1).any() and anti1.any(1).all()
  _assert_rows_alive(psi, rows1.reshape(-1, n), tag + ' single exchanges')
  _assert_rows_alive(psi, rows2.reshape(-1, n), tag + ' double exchanges')
  assert (own_psi != 0).all() and np.isfinite(own_psi).all()
  bond_sum, dd_sum = eng.dimer_correlations(bonds, pairs)
  # (1) the oracle
  bond_ref, dd_ref, bond_bound, dd_bound = td._reference(psi, eps, cfg, bonds, pairs)
  td._check(tag + ' bond_sum', bond_sum, bond_ref, bond_bound)
  td._check(tag + ' dd_sum', dd_sum, dd_ref, dd_bound)
  # (2) the library's own rows, folded as k_dimer_bond_fold / k_dimer_fold fold them (the products are by powers of two)
  own = eng.amplitude()[0].astype(np.float64)
  l1 = eng.amplitude(rows1.reshape(-1, n))[0].astype(np.float64).reshape(len(bonds), B)
  l2 = eng.amplitude(rows2.reshape(-1, n))[0].astype(np.float64).reshape(len(pairs), B)
  r1 = np.where(anti1, np.exp(l1 - own[None, :]), 0.0)                  # r(swap_ij x) per (bond, chain)
  r2 = np.where(anti2, np.exp(l2 - own[None, :]), 0.0)                  # r(swap_kl swap_ij x) per (pair, chain)
  zz = np.array([0.25 * cfg[:, i].astype(np.float64) * cfg[:, j] for i, j in bonds])
  bond_terms = zz + 0.5 * r1
  _own_rows_check(tag + ' bond_sum', bond_sum, _ascending(bond_terms), (np.abs(zz) + 0.5 * np.abs(r1)).sum(1))
  dd_terms, dd_abs = np.zeros((len(pairs), B)), np.zeros(len(pairs))
  for p, (a, b) in enumerate(pairs):
    inner = zz[b] + 0.5 * r1[b]
    term = zz[a] * inner
    outer = 0.25 * spins2[p] * r1[a] + 0.5 * r2[p]
    dd_terms[p] = np.where(anti1[a], term + 0.5 * outer, term)
    dd_abs[p] = (np.abs(zz[a]) * (np.abs(zz[b]) + 0.5 * np.abs(r1[b])) + anti1[a] * (0.125 * np.abs(r1[a]) + 0.25 * np.abs(r2[p]))).sum()
  _own_rows_check(tag + ' dd_sum', dd_sum, _ascending(dd_terms), dd_abs)
  if splits:
    for per in (0, 1, 7):
      for _ in range(2):
        bs, dd = eng.dimer_correlations(bonds, pairs, pairs_per_pass=per)
        np.testing.assert_array_equal(bs, bond_sum, err_msg='pairs_per_pass=%d' % per)
        np.testing.assert_array_equal(dd, dd_sum, err_msg='pairs_per_pass=%d' % per)
    # the request splits the single exchanges too: one `dimer_rows` region per pass of either phase
    eng.timing_enable(True); eng.timing_reset()
    bs, dd = eng.dimer_correlations(bonds, pairs, pairs_per_pass=7)
    eng.synchronize()
    passes = eng.timing_get('dimer_rows')[1]
    eng.timing_enable(False)
    assert passes == (len(bonds) + 6) // 7 + (len(pairs) + 6) // 7, passes
    np.testing.assert_array_equal(bs, bond_sum); np.testing.assert_array_equal(dd, dd_sum)


def _check_corr(tag, eng, psi, cfg, n, splits):
  pairs = _site_pairs(n)
  assert len(pairs) > 256
  zz, ex = eng.pair_correlations(pairs)
  # (1) the oracle: tests/test_gpu_corr.py's bound of the dense and convolutional types on the per-pair means
  ref_zz, ref_ex = co.pair_sums(psi, cfg, pairs)
  np.testing.assert_array_equal(zz, ref_zz)
  for name, got, ref in (('exchange', 0.5 * ex / B, 0.5 * ref_ex / B), ('ss', (0.25 * zz + 0.5 * ex) / B, (0.25 * ref_zz + 0.5 * ref_ex) / B)):
    bound = 2e-4 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref)
    print('%s pair means %s: worst error / bound %.3g (pair %s)' % (tag, name, err.max() / bound, tuple(pairs[err.argmax()])))
    assert (err <= bound).all(), (name, tuple(pairs[err.argmax()]), err.max(), bound)
  # (2) the fold against the host sum of the library's own fp32 rows: one single-bond Hamiltonian per pair (the boundary
  # pairs and a few of the others), one row per antiparallel chain
  worst = 0.0
  for k in (0, 1, 2, 3, 50, 200, len(pairs) - 1):
    eng.set_bonds([tuple(pairs[k])], 2.0, 0.0)
    diag, rows = eng.local_energy_terms()
    anti = cfg[:, pairs[k, 0]] != cfg[:, pairs[k, 1]]
    assert (diag == 0).all() and (rows[~anti] == 0).all()
    host = 0.0
    for v in rows.astype(np.float64):
      host += v
    bound = B * 2.0 ** -53 * np.abs(rows.astype(np.float64)).sum()
    assert abs(ex[k] - host) <= bound, (k, ex[k], host, bound)
    worst = max(worst, abs(ex[k] - host) / bound if bound > 0 else 0.0)
  print('%s pair fold vs the host sum of the rows: worst |diff| / bound %.3g' % (tag, worst))
  assert (cfg[:, pairs[:4, 0]] != cfg[:, pairs[:4, 1]]).any(0).all()    # every boundary pair has rows
  if splits:
    for per in (0, 1, 7):
      for _ in range(2):
        z, e = eng.pair_correlations(pairs, pairs_per_pass=per)
        np.testing.assert_array_equal(z, zz, err_msg='pairs_per_pass=%d' % per)
        np.testing.assert_array_equal(e, ex, err_msg='pairs_per_pass=%d' % per)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_measurements_beyond_64_sites(monkeypatch, case):
  tag, ansatz, n, h, L, path, general, splits = case
  theta, psi, eps = _family(ansatz, n, h, L)
  cfg = vo.random_configurations(n, B, np.random.RandomState(3))
  assert (cfg.sum(1) == 0).all()
  eng = _engine(ansatz, n, h, L, general, monkeypatch)
  assert eng.kernel_path() == path
  eng.set_params(theta); eng.set_configs(cfg)
  _check_renyi(tag, eng, psi, eps, cfg, n, splits)
  _check_dimer(tag, eng, psi, eps, cfg, n, splits)
  _check_corr(tag, eng, psi, cfg, n, splits)
  eng.close()

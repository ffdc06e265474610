"""GPU: the local-energy form of the patch kernel (csrc/conv_patch.hip, k_cgen_patch_sweep<..., ELOC>) on rows that are no
nearest-neighbour bonds -- J1-J2 bond sets (vmc_set_bonds) and arbitrary site pairs (vmc_set_bonds, vmc_pair_correlations),
the class lists of tests/pair_classes.py (held to what they claim by tests/test_pair_classes.py on the CPU): merged boxes
along an axis and along a diagonal, the diagonal that must not merge (K = 2), two boxes that share sites, abut or lie
apart, pairs across the row-major seam, the D / 2 tie, (j, i) against (i, j).

Checks: bit equality with a full forward of every row (CGS_VMC_CONV_PATCH=0, read per call) and the fp64 oracle at the
bounds of tests/test_gpu_conv_general.py (2e-4 max(1, |ref|) per local value) and tests/test_gpu_corr.py
(2e-4 max(1, max|ref|) on the per-pair means).  At 36 x 36 the oracle's amplitudes leave the doubles: the bits are the
check there, as in test_patch_rows_give_the_local_energies_of_the_full_forward."""
import numpy as np
import pytest

from cgs_vmc_amd import _hip
from oracle import vmc_oracle as vo
from tests import corr_oracle as co
from tests import pair_classes as pc
from tests.test_gpu_conv import _close, _make
from tests.test_gpu_conv_general import PATCH_SHAPES

pytestmark = pytest.mark.gpu
IDS = ['{}-{}x{}-L{}-F{}-K{}-B{}-{}'.format(*s) for s in PATCH_SHAPES]
TWO_D = [s for s in PATCH_SHAPES if s[0] not in vo.CONV_1D]
IDS_2D = ['{}-{}x{}-L{}-F{}-K{}-B{}-{}'.format(*s) for s in TWO_D]


def _j1j2(sx, sy):
  """Nearest neighbours (J1 = 1) and both diagonals (J2 = 0.5) of the torus, per-bond couplings (site = a2 + size_y a1)."""
  bonds = vo.torus_bonds(sy, sx, next_nearest=True)
  j = np.concatenate([np.ones(len(bonds) // 2), 0.5 * np.ones(len(bonds) // 2)]).astype(np.float32)
  return bonds, -j, j


def _hamiltonian(ansatz, sx, sy):
  if ansatz in vo.CONV_1D:
    return vo.chain_bonds(sx * sy), -1.0, 1.0
  return _j1j2(sx, sy)


def _chains_for(pairs, n, b, seed):
  """b configurations (Sz = 0; one spin over on an odd lattice) in which every pair of `pairs` is antiparallel -- exchanged, a row of the patch kernel -- in
  at least one chain: pair number p is made antiparallel in chain p mod b by exchanging one of its sites with a site of
  the opposite spin that no earlier pair of that chain has used."""
  cfg = vo.random_configurations(n, b, np.random.RandomState(seed))
  total = cfg.sum(1)
  fixed = [set() for _ in range(b)]
  for p, (i, j) in enumerate(pairs):
    c = p % b
    row = cfg[c]
    if row[i] == row[j]:
      move = j if j not in fixed[c] else (i if i not in fixed[c] else None)
      if move is not None:
        k = next(k for k in range(n) if k not in fixed[c] and k not in (i, j) and row[k] != row[move])
        row[move], row[k] = row[k], row[move]
    fixed[c] |= {i, j}
  assert (cfg.sum(1) == total).all()
  assert all((cfg[:, i] != cfg[:, j]).any() for i, j in pairs)
  return cfg


def _setup(monkeypatch, shape):
  ansatz, sx, sy, L, f, k, b, nonlin = shape
  monkeypatch.setenv('CGS_VMC_CONV_GENERAL', '1')
  eng, theta, cfg, bonds, geom = _make(*shape)
  assert eng.kernel_path() == 6
  classes = pc.class_pairs(pc.geometry(ansatz, sx, sy, L, k))
  pairs = pc.bonds_of(classes)
  amp = lambda c: vo.ANSATZ[ansatz][0](theta, c, geom, L, nonlinearity=nonlin, dtype=np.float64)
  return eng, theta, amp, classes, pairs


@pytest.mark.parametrize('shape', TWO_D, ids=IDS_2D)
def test_j1j2_local_energies_through_the_patch_rows(monkeypatch, shape):
  ansatz, sx, sy, L, f, k, b, nonlin = shape
  monkeypatch.setenv('CGS_VMC_CONV_GENERAL', '1')
  eng, theta, cfg, _, geom = _make(*shape)
  assert eng.kernel_path() == 6
  bonds, jx, jz = _j1j2(sx, sy)
  assert len(bonds) == 4 * sx * sy
  eng.set_bonds(bonds, jx, jz)
  out = {}
  for patch in ('0', '2'):
    monkeypatch.setenv('CGS_VMC_CONV_PATCH', patch)
    eng.set_configs(cfg)
    eloc, mean = eng.local_energy()
    diag, off = eng.local_energy_terms()
    eng.reset_accumulators()
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    out[patch] = (eloc, np.float64(mean), diag, off, eng.get_accumulators())
  assert eng.last_connected_rows() > b
  for a, bb in zip(out['0'], out['2']):
    np.testing.assert_array_equal(a, bb)
  if sx * sy <= 1000:
    amp = lambda c: vo.ANSATZ[ansatz][0](theta, c, geom, L, nonlinearity=nonlin, dtype=np.float64)
    ref = vo.local_value(amp, cfg, bonds, jx, jz, dtype=np.float64)
    err = np.abs(out['2'][0] - ref) / (2e-4 * np.maximum(1.0, np.abs(ref)))
    print('%s J1-J2 local energies: worst error / bound %.3g' % (IDS_2D[TWO_D.index(shape)], err.max()))
    _close(out['2'][0], ref, 2e-4)
  eng.close()


@pytest.mark.parametrize('shape', PATCH_SHAPES, ids=IDS)
def test_arbitrary_pairs_as_a_bond_set(monkeypatch, shape):
  ansatz, sx, sy, L, f, k, b, nonlin = shape
  n = sx * sy
  eng, theta, amp, classes, pairs = _setup(monkeypatch, shape)
  cfg = _chains_for(pairs, n, b, 11)
  oracle = n <= 1000
  own = amp(cfg) if oracle else None
  # the whole list as one bond set: j_x = 2, j_z = 0 makes a chain's off-diagonal term the sum of its rows' bare ratios
  eng.set_bonds(pairs, 2.0, 0.0)
  out = {}
  for patch in ('0', '2'):
    monkeypatch.setenv('CGS_VMC_CONV_PATCH', patch)
    eng.set_configs(cfg)
    eloc = eng.local_energy()[0]
    out[patch] = eng.local_energy_terms() + (eloc,)
  assert eng.last_connected_rows() > b
  for a, bb in zip(out['0'], out['2']):
    np.testing.assert_array_equal(a, bb)
  assert (out['2'][0] == 0).all()
  if oracle:
    _, ratio = co.pair_terms(amp, cfg, pairs)
    _close(out['2'][1], ratio.sum(1), 2e-4)
  # row by row: one pair as the bond set, a chain's term is that row's psi(swap x) / psi(x)
  worst = 0.0
  for name, i, j in classes:
    eng.set_bonds([(i, j)], 2.0, 0.0)
    rows = {}
    for patch in ('0', '2'):
      monkeypatch.setenv('CGS_VMC_CONV_PATCH', patch)
      eng.set_configs(cfg)
      rows[patch] = eng.local_energy_terms()[1]
    np.testing.assert_array_equal(rows['0'], rows['2'], err_msg='%s (%d, %d)' % (name, i, j))
    anti = cfg[:, i] != cfg[:, j]
    assert anti.any() and (rows['2'][~anti] == 0).all(), name
    if oracle:
      swapped = cfg[anti].copy()
      swapped[:, [i, j]] = swapped[:, [j, i]]
      ref = np.zeros(b)
      ref[anti] = amp(swapped) / own[anti]
      worst = max(worst, (np.abs(rows['2'] - ref) / (2e-4 * np.maximum(1.0, np.abs(ref)))).max())
      try:
        _close(rows['2'], ref, 2e-4)
      except AssertionError as e:
        raise AssertionError('%s (%d, %d): %s' % (name, i, j, e))
  if oracle:
    print('%s pair rows: worst error / bound %.3g' % (IDS[PATCH_SHAPES.index(shape)], worst))
  eng.close()


@pytest.mark.parametrize('shape', PATCH_SHAPES, ids=IDS)
def test_the_same_pairs_through_pair_correlations(monkeypatch, shape):
  ansatz, sx, sy, L, f, k, b, nonlin = shape
  n = sx * sy
  eng, theta, amp, classes, pairs = _setup(monkeypatch, shape)
  cfg = _chains_for(pairs, n, b, 12)
  ij = np.array(pairs)
  h_bonds, jx, jz = _hamiltonian(ansatz, sx, sy)
  eng.set_bonds(h_bonds, jx, jz)
  eng.set_configs(cfg)
  monkeypatch.setenv('CGS_VMC_CONV_PATCH', '2')
  before = (eng.local_energy()[0],) + eng.local_energy_terms()
  ref_zz = (cfg[:, ij[:, 0]].astype(np.int64) * cfg[:, ij[:, 1]].astype(np.int64)).sum(0)
  out = {}
  for patch in ('0', '2'):
    monkeypatch.setenv('CGS_VMC_CONV_PATCH', patch)
    out[patch] = eng.pair_correlations(pairs)
    np.testing.assert_array_equal(out[patch][0], ref_zz.astype(np.float64))
  np.testing.assert_array_equal(out['0'][1], out['2'][1])
  for per in (0, 1, 5):
    zz, ex = eng.pair_correlations(pairs, pairs_per_pass=per)
    np.testing.assert_array_equal(zz, out['2'][0], err_msg='pairs_per_pass=%d' % per)
    np.testing.assert_array_equal(ex, out['2'][1], err_msg='pairs_per_pass=%d' % per)
  # the Hamiltonian's set answers with the bits it gave before the measurements
  after = (eng.local_energy()[0],) + eng.local_energy_terms()
  for x, y in zip(before, after):
    np.testing.assert_array_equal(x, y)
  if n <= 1000:
    _, ref_exch, ref_ss = co.pair_means(amp, cfg, pairs)
    zz, ex = out['2']
    for name, got, ref in (('exchange', 0.5 * ex / b, ref_exch), ('ss', (0.25 * zz + 0.5 * ex) / b, ref_ss)):
      bound = 2e-4 * max(1.0, np.abs(ref).max())
      err = np.abs(got - ref)
      print('%s %s: worst error / bound %.3g (pair %s)' % (IDS[PATCH_SHAPES.index(shape)], name, err.max() / bound, classes[int(err.argmax())]))
      assert (err <= bound).all(), (name, classes[int(err.argmax())], err.max(), bound)
  eng.close()


def test_default_routing_sends_a_measurement_to_the_patch_rows(monkeypatch):
  """No patch or general variable: plan_desc routes 20 x 20, 3 x 16 filters 3 x 3 to the general path, and a pass of at
  least 4 B rows takes the patch kernel by itself -- the class list and the J1-J2 bonds as the pairs of one measurement."""
  ansatz, sx, sy, L, f, k, b, nonlin = shape = ('conv_2d', 20, 20, 3, 16, 3, 6, 'relu')
  for var in ('CGS_VMC_CONV_GENERAL', 'CGS_VMC_CONV_PATCH'):
    monkeypatch.delenv(var, raising=False)
  n = sx * sy
  eng, theta, _, _, geom = _make(*shape)
  assert eng.kernel_path() == 6 and eng.conv_patch(n)
  amp = lambda c: vo.ANSATZ[ansatz][0](theta, c, geom, L, nonlinearity=nonlin, dtype=np.float64)
  classes = pc.class_pairs(pc.geometry(ansatz, sx, sy, L, k))
  pairs = pc.bonds_of(classes) + [tuple(x) for x in _j1j2(sx, sy)[0]]
  cfg = _chains_for(pc.bonds_of(classes), n, b, 13)
  eng.set_configs(cfg)
  ij = np.array(pairs)
  anti = cfg[:, ij[:, 0]] != cfg[:, ij[:, 1]]
  assert anti.sum() >= 4 * b                           # the rows of the one pass: beyond the threshold of cgen_forward
  zz, ex = eng.pair_correlations(pairs)
  np.testing.assert_array_equal(zz, (cfg[:, ij[:, 0]].astype(np.int64) * cfg[:, ij[:, 1]].astype(np.int64)).sum(0).astype(np.float64))
  _, ref_exch, ref_ss = co.pair_means(amp, cfg, pairs)
  for name, got, ref in (('exchange', 0.5 * ex / b, ref_exch), ('ss', (0.25 * zz + 0.5 * ex) / b, ref_ss)):
    bound = 2e-4 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref)
    print('default routing %s: worst error / bound %.3g (pair %s)' % (name, err.max() / bound, pairs[int(err.argmax())]))
    assert (err <= bound).all(), (name, pairs[int(err.argmax())], err.max(), bound)
  # the same bits with a full forward of every row
  monkeypatch.setenv('CGS_VMC_CONV_PATCH', '0')
  zz0, ex0 = eng.pair_correlations(pairs)
  np.testing.assert_array_equal(zz0, zz); np.testing.assert_array_equal(ex0, ex)
  eng.close()

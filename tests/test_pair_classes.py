"""CPU guard of tests/pair_classes.py: for every row of PATCH_SHAPES the class list really holds what the GPU tests
(tests/test_gpu_patch_pairs.py) claim to send through the local-energy form of the patch kernel -- every class the shape
admits, rows with one merged box and rows with two, diagonals merged exactly where the kernel's rule merges them."""
import pytest

from tests import pair_classes as pc
from tests.test_gpu_conv_general import PATCH_SHAPES

IDS = ['{}-{}x{}-L{}-F{}-K{}-B{}-{}'.format(*s) for s in PATCH_SHAPES]
DEFAULT_ROUTED = ('conv_2d', 20, 20, 3, 16, 3, 6, 'relu')      # the shape plan_desc routes by itself


def _geom(shape):
  ansatz, sx, sy, L, f, k, b, nonlin = shape
  return pc.geometry(ansatz, sx, sy, L, k)


@pytest.mark.parametrize('shape', PATCH_SHAPES + [DEFAULT_ROUTED], ids=IDS + ['default-routed'])
def test_class_list_reaches_every_branch_of_the_merge_rule(shape):
  geom = _geom(shape)
  d1, d2, k, kw, n_conv = geom
  n = d1 * d2
  pairs = pc.class_pairs(geom)
  names = [name for name, _, _ in pairs]
  assert len(pairs) <= 36 and len(set(names)) == len(names)
  assert len({(i, j) for _, i, j in pairs}) == len(pairs)                 # no ordered pair twice
  for name, i, j in pairs:
    assert 0 <= i < n and 0 <= j < n and i != j, (name, i, j)
  # every admissible class is there, with the displacement its name promises
  admitted = pc.class_displacements(geom)
  by_name = {name: (i, j) for name, i, j in pairs}
  for name, d in admitted:
    assert name in by_name and pc.displacement(*by_name[name], geom) == d, (name, d)
  two_d = d2 > 1
  must = ['axis1', 'two1', 'seam1'] + (['axis2', 'diag+', 'diag-', 'two2', 'knight12', 'knight21', 'seam2', 'seamdiag'] if two_d else [])
  if d1 % 2 == 0:
    must.append('half1')
  if two_d and d1 % 2 == 0 and d2 % 2 == 0:
    must.append('halfhalf')
  s1, s2 = pc.box_side(geom, 0), pc.box_side(geom, 1)
  if 2 * s1 <= d1:
    must.append('touch1')
  if 2 * s1 + 1 <= d1:
    must.append('apart1')
  if two_d and 2 * s2 <= d2:
    must.append('touch2')
  if two_d and 2 * s2 + 1 <= d2:
    must.append('apart2')
  assert not set(must) - set(names), set(must) - set(names)
  assert sum(name.startswith('rev:') for name in names) >= 3
  for name, i, j in pairs:
    if name.startswith('rev:'):
      assert by_name[name[4:]] == (j, i)
  # both forms of a row occur
  nbx = {name: pc.merge(i, j, geom) for name, i, j in pairs}
  assert {v[0] for v in nbx.values()} == {1, 2}
  # the seam pairs are neighbours round the torus
  assert pc.displacement(*by_name['seam1'], geom) == (-1, 0)
  if two_d:
    assert pc.displacement(*by_name['seam2'], geom) == (0, -1) and pc.displacement(*by_name['seamdiag'], geom) == (-1, -1)
  # a diagonal is merged exactly when (K + 1)(KW + 1) <= 2 K KW and the merged last box fits the lattice
  if two_d:
    expect = (k + 1) * (kw + 1) <= 2 * k * kw and s1 + 1 <= d1 and s2 + 1 <= d2
    for name in ('diag+', 'diag-', 'seamdiag'):
      assert nbx[name] == ((1, 1, 1) if expect else (2, 0, 0)), (name, nbx[name])
  # an axis neighbour merges where its box fits ((K + 1) KW <= 2 K KW always)
  assert nbx['axis1'] == ((1, 1, 0) if s1 + 1 <= d1 else (2, 0, 0))
  assert nbx['rev:axis1'] == nbx['axis1'] and nbx['seam1'] == nbx['axis1']
  if two_d:
    assert nbx['axis2'] == ((1, 0, 1) if s2 + 1 <= d2 else (2, 0, 0))
  # nothing further apart merges, and the two-box rows cover boxes that share sites, that abut and that are apart
  for name, i, j in pairs:
    dy, dx = pc.displacement(i, j, geom)
    if max(abs(dy), abs(dx)) > 1:
      assert nbx[name][0] == 2
  kinds = {name: pc.overlap(i, j, geom) for name, i, j in pairs if nbx[name][0] == 2}
  assert kinds['two1'] == 'partial'
  for axis in ('1', '2'):
    if 'touch' + axis in names:
      assert kinds['touch' + axis] == 'touch'
    if 'apart' + axis in names:
      assert kinds['apart' + axis] == 'disjoint'


def test_displacement_takes_the_shorter_way_and_breaks_the_tie_upwards():
  geom = (6, 5, 3, 3, 2)
  site = lambda a1, a2: a1 * 5 + a2
  assert pc.displacement(site(0, 0), site(5, 4), geom) == (-1, -1)
  assert pc.displacement(site(5, 4), site(0, 0), geom) == (1, 1)
  assert pc.displacement(site(1, 1), site(4, 1), geom) == (3, 0)          # D1 / 2 on the even side: +3 ...
  assert pc.displacement(site(4, 1), site(1, 1), geom) == (3, 0)          # ... from either end
  assert pc.displacement(site(0, 0), site(0, 3), geom) == (0, -2)         # odd side: no tie
  assert pc.displacement(site(0, 3), site(0, 0), geom) == (0, 2)
  # K = 2: the diagonal's merged first box (3 x 3 = 9) is larger than the two it replaces (8)
  assert pc.merge(7, 14, (6, 6, 2, 2, 2)) == (2, 0, 0)                    # (1, 1) and (2, 2) on six columns
  assert pc.merge(7, 8, (6, 6, 2, 2, 2)) == (1, 0, 1)
  assert pc.merge(site(1, 1), site(2, 2), geom) == (2, 0, 0)              # 5 + 1 > 5 along axis 2: does not fit
  assert pc.merge(7, 14, (6, 6, 3, 3, 2)) == (1, 1, 1)

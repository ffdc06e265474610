"""Site pairs by geometric class for the local-energy form of the patch kernel (csrc/conv_patch.hip, k_cgen_patch_sweep<..., ELOC>).

The kernel decides per row whether the two exchanged sites get ONE merged bounding box per convolution (nbx = 1, e1 / e2 =
the displacement) or two boxes (nbx = 2).  This file restates that rule in plain Python from the geometry
(D1, D2, K, KW, n_conv) -- displacement(), merge() -- and class_pairs() returns, for a shape, a short list of pairs with at
least one of every class the shape admits: tests/test_pair_classes.py holds the list to that on the CPU, the GPU tests
(tests/test_gpu_patch_pairs.py) send it through vmc_set_bonds and vmc_pair_correlations.

Sites are row-major, site = a1 * D2 + a2 (D1 = size_x, D2 = size_y; the 1-D types live on D1 = n, D2 = 1 with KW = 1).
Test infrastructure; nothing here is used by the product path."""

CONV_1D = ('conv_1d', 'res_net_1d')


def geometry(ansatz, sx, sy, num_layers, k):
  """(D1, D2, K, KW, n_conv) as plan_desc fills ConvGeom (plan.hpp): residual networks have 1 + 2 blocks convolutions."""
  n_conv = 1 + 2 * num_layers if ansatz.startswith('res_net') else num_layers
  return (sx, sy, k, 1 if ansatz in CONV_1D else k, n_conv)


def box_side(geom, axis):
  """Sites per axis of the LAST convolution's box around one changed site: n_conv (K - 1) + 1."""
  d1, d2, k, kw, n_conv = geom
  return n_conv * ((kw if axis else k) - 1) + 1


def displacement(i, j, geom):
  """(dy, dx): site j from site i, the shorter way round the torus; a tie (|d| = D / 2 on an even side) counts as +D / 2."""
  d1, d2 = geom[0], geom[1]
  dy = j // d2 - i // d2
  dx = j % d2 - i % d2
  if dy > d1 // 2:
    dy -= d1
  elif dy < -((d1 - 1) // 2):
    dy += d1
  if dx > d2 // 2:
    dx -= d2
  elif dx < -((d2 - 1) // 2):
    dx += d2
  return dy, dx


def merge(i, j, geom):
  """(nbx, e1, e2) of the row that exchanges sites i and j: one merged box where the sites are at most one step apart along
  each axis, the merged last box fits the lattice and the merged first box is no larger than the two it replaces."""
  d1, d2, k, kw, n_conv = geom
  dy, dx = displacement(i, j, geom)
  ady, adx = abs(dy), abs(dx)
  merged = (ady <= 1 and adx <= 1 and box_side(geom, 0) + ady <= d1 and box_side(geom, 1) + adx <= d2 and
            (k + ady) * (kw + adx) <= 2 * k * kw)
  return (1, ady, adx) if merged else (2, 0, 0)


def boxes(i, j, geom):
  """The two last-convolution boxes as sets of (a1, a2) (the box of a site q reaches n_conv taps to either side in total;
  where it starts does not matter for whether two boxes of the same network meet: both start the same way)."""
  d1, d2 = geom[0], geom[1]
  s1, s2 = box_side(geom, 0), box_side(geom, 1)
  out = []
  for q in (i, j):
    a1, a2 = q // d2, q % d2
    out.append({((a1 + u) % d1, (a2 + v) % d2) for u in range(s1) for v in range(s2)})
  return out


def overlap(i, j, geom):
  """'full' never happens for distinct sites; 'partial' (the boxes share sites), 'touch' (no shared site, but a site of one
  is a lattice neighbour of a site of the other) or 'disjoint'."""
  d1, d2 = geom[0], geom[1]
  a, b = boxes(i, j, geom)
  if a & b:
    return 'partial'
  near = {((y + u) % d1, (x + v) % d2) for (y, x) in a for (u, v) in ((1, 0), (-1, 0), (0, 1), (0, -1))}
  return 'touch' if near & b else 'disjoint'


def _site(a1, a2, geom):
  d1, d2 = geom[0], geom[1]
  return (a1 % d1) * d2 + (a2 % d2)


def class_displacements(geom):
  """[(class name, (dy, dx))] the shape admits: a displacement is admitted where it is its own shorter way round (so that
  the class means what its name says) and leaves two distinct sites."""
  d1, d2 = geom[0], geom[1]
  s1, s2 = box_side(geom, 0), box_side(geom, 1)
  want = [('axis1', (1, 0)), ('axis2', (0, 1)), ('diag+', (1, 1)), ('diag-', (1, -1)),
          ('two1', (2, 0)), ('two2', (0, 2)), ('knight12', (1, 2)), ('knight21', (2, 1))]
  # the last convolution's boxes side by side along an axis: abutting (same columns, no shared site), then one site apart
  if 2 * s1 <= d1:
    want.append(('touch1', (s1, 0)))
  if 2 * s1 + 1 <= d1:
    want.append(('apart1', (s1 + 1, 0)))
  if d2 > 1 and 2 * s2 <= d2:
    want.append(('touch2', (0, s2)))
  if d2 > 1 and 2 * s2 + 1 <= d2:
    want.append(('apart2', (0, s2 + 1)))
  if d1 % 2 == 0:
    want.append(('half1', (d1 // 2, 0)))
  if d1 % 2 == 0 and d2 % 2 == 0:
    want.append(('halfhalf', (d1 // 2, d2 // 2)))
  out = []
  for name, (dy, dx) in want:
    if d2 == 1 and dx != 0:
      continue
    if abs(dy) > d1 // 2 or abs(dx) > d2 // 2 or (dy, dx) == (0, 0):
      continue
    out.append((name, (dy, dx)))
  return out


def class_pairs(geom):
  """[(class name, i, j)]: every admitted class from anchors spread over the lattice (interior, the last row and column, so
  that windows and boxes wrap), the pairs across the row-major seam, and three classes again as (j, i)."""
  d1, d2 = geom[0], geom[1]
  anchors = [(1, 1), (d1 - 1, d2 - 1), (0, d2 // 2), (d1 // 2, 0), (d1 - 2, 2)]
  out = []
  for n, (name, (dy, dx)) in enumerate(class_displacements(geom)):
    a1, a2 = anchors[n % len(anchors)]
    out.append((name, _site(a1, a2, geom), _site(a1 + dy, a2 + dx, geom)))
  # the row-major seam: first row with last row, first column with last column (neighbours round the torus), and the corner
  out.append(('seam1', _site(0, d2 // 3, geom), _site(d1 - 1, d2 // 3, geom)))
  if d2 > 1:
    out.append(('seam2', _site(d1 // 3, 0, geom), _site(d1 // 3, d2 - 1, geom)))
    out.append(('seamdiag', _site(0, 0, geom), _site(d1 - 1, d2 - 1, geom)))
  # (j, i) against (i, j): an axis neighbour, a diagonal (or the second listed class in 1-D) and a far pair
  by_name = {name: (i, j) for name, i, j in out}
  for name in ('axis1', 'diag-' if 'diag-' in by_name else 'two1', 'seam1', out[len(class_displacements(geom)) - 1][0]):
    i, j = by_name[name]
    if ('rev:' + name, j, i) not in out:
      out.append(('rev:' + name, j, i))
  return out


def bonds_of(pairs):
  return [(i, j) for _, i, j in pairs]

"""fp64 restatement of GraphConvNetwork (wavefunctions.py:1083-1154; layers.GraphConvLayer,
layers.py:415-451) for the tests, plus the adjacency lists they use.

A layer gathers x[:, adj] -> [B, N, k, Cin] and applies snt.Conv2D with a 1 x k kernel, VALID
padding and a bias: z[b, n, o] = bias[o] + sum_{t, c} x[b, adj[n, t], c] w[0, t, c, o].  Every
layer but the last is followed by the nonlinearity; the logit is the sum of the last map.  The
sampler, the Hamiltonian, the accumulators and SR come from oracle.vmc_oracle through an amp_fn.
"""
import numpy as np

from oracle import vmc_oracle as vo


# --------------------------------------------------------------------------- adjacency lists
def stencil_adjacency(sx, sy, k):
  """The k x k periodic stencil of Conv2dPeriodic on an sx x sy torus in the tap order of the
  general path's gather (conv_general.hip cg_site): tap t = d1 k + d2 of position (a1, a2) reads
  ((a1 + d1 - lo) mod sx, (a2 + d2 - lo) mod sy), lo = (k - 1) // 2 (layers.py:132-141)."""
  lo = (k - 1) // 2
  adj = np.zeros((sx * sy, k * k), np.int32)
  for a1 in range(sx):
    for a2 in range(sy):
      for d1 in range(k):
        for d2 in range(k):
          adj[a1 * sy + a2, d1 * k + d2] = ((a1 + d1 - lo) % sx) * sy + (a2 + d2 - lo) % sy
  return adj


def square_5point_adjacency(sx, sy):
  """Self and the four nearest neighbours on an sx x sy torus (k = 5)."""
  adj = []
  for a1 in range(sx):
    for a2 in range(sy):
      s = lambda i, j: ((a1 + i) % sx) * sy + (a2 + j) % sy
      adj.append([s(0, 0), s(-1, 0), s(1, 0), s(0, -1), s(0, 1)])
  return np.asarray(adj, np.int32)


def triangular_adjacency(lx, ly):
  """Self and the six neighbours of the triangular lattice on an lx x ly torus (k = 7)."""
  adj = []
  for a1 in range(lx):
    for a2 in range(ly):
      s = lambda i, j: ((a1 + i) % lx) * ly + (a2 + j) % ly
      adj.append([s(0, 0), s(1, 0), s(-1, 0), s(0, 1), s(0, -1), s(1, -1), s(-1, 1)])
  return np.asarray(adj, np.int32)


def triangular_bonds(lx, ly):
  bonds = set()
  for a1 in range(lx):
    for a2 in range(ly):
      i = a1 * ly + a2
      for d1, d2 in ((1, 0), (0, 1), (1, -1)):
        j = ((a1 + d1) % lx) * ly + (a2 + d2) % ly
        if i != j:
          bonds.add((min(i, j), max(i, j)))
  return sorted(bonds)


def honeycomb_adjacency(lx, ly):
  """Self and the three neighbours of the honeycomb lattice on an lx x ly torus of two-site cells
  (2 lx ly sites, k = 4); site 2 (a1 ly + a2) + s, sublattice s."""
  idx = lambda a1, a2, s: 2 * ((a1 % lx) * ly + a2 % ly) + s
  adj = []
  for a1 in range(lx):
    for a2 in range(ly):
      adj.append([idx(a1, a2, 0), idx(a1, a2, 1), idx(a1 - 1, a2, 1), idx(a1, a2 - 1, 1)])
      adj.append([idx(a1, a2, 1), idx(a1, a2, 0), idx(a1 + 1, a2, 0), idx(a1, a2 + 1, 0)])
  return np.asarray(adj, np.int32)


def ring_adjacency(n):
  """Self and the next site of a ring (k = 2, the smallest table the planner takes)."""
  return np.stack([np.arange(n), (np.arange(n) + 1) % n], 1).astype(np.int32)


def random_adjacency(n, k, rng, self_first=False):
  """Entries uniform over the sites (repeats within a row, uneven in-degrees); self_first: column 0 is the site."""
  adj = rng.integers(0, n, size=(n, k)).astype(np.int32)
  if self_first:
    adj[:, 0] = np.arange(n)
  return adj


def hub_adjacency(n, k):
  """Column 0 is the site, every other tap of every row is site 0: one inverse list of n (k - 1) + 1 entries next to
  n - 1 lists of one."""
  adj = np.zeros((n, k), np.int32)
  adj[:, 0] = np.arange(n)
  return adj


def empty_list_adjacency(n, k, n_read, rng):
  """The last n - n_read sites appear in NO row (empty inverse lists: their input gradient is 0): rows of the first
  n_read sites are the site and k - 1 uniform draws below n_read, the other rows k uniform draws below n_read."""
  adj = rng.integers(0, n_read, size=(n, k)).astype(np.int32)
  adj[:n_read, 0] = np.arange(n_read)
  return adj


def irregular_adjacency():
  """12 sites, k = 5: repeated entries within a row, tap columns that are not permutations (site 0 is read by
  many taps, sites 10 / 11 by few), a site nobody reads but itself (k_gnn_col2im's uneven inverse lists)."""
  rng = np.random.default_rng(5)
  adj = rng.integers(0, 10, size=(12, 5)).astype(np.int32)
  adj[:, 0] = np.arange(12)
  adj[::3, 2] = 0
  adj[1, 3] = adj[1, 4] = 7
  return adj


def in_degree(adj):
  """How many (position, tap) pairs read each site: the lengths of plan_gnn_inverse's lists."""
  return np.bincount(np.asarray(adj).ravel(), minlength=np.asarray(adj).shape[0])


def adjacency_bonds(adj):
  """The distinct undirected pairs (i, j), i != j, of a table."""
  bonds = set()
  for n, row in enumerate(adj):
    for s in row:
      if s != n:
        bonds.add((min(n, int(s)), max(n, int(s))))
  return sorted(bonds)


# --------------------------------------------------------------------------- parameters
def gnn_param_shapes(k, f, num_layers):
  shapes, cin = [], 1
  for _ in range(num_layers):
    shapes += [(1, k, cin, f), (f,)]
    cin = f
  return shapes


def gnn_num_params(k, f, num_layers):
  return int(sum(int(np.prod(s)) for s in gnn_param_shapes(k, f, num_layers)))


def gnn_init_params(k, f, num_layers, rng, noise=0.03):
  """snt.Conv2D's init (sigma = 1 / sqrt(k Cin)) plus a little noise, so that biases are non-zero."""
  parts = []
  for shp in gnn_param_shapes(k, f, num_layers):
    if len(shp) == 4:
      w = np.clip(rng.standard_normal(shp), -2, 2) / np.sqrt(shp[1] * shp[2])
      parts.append(w.ravel())
    else:
      parts.append(np.zeros(shp))
  theta = np.concatenate(parts)
  return (theta + noise * rng.standard_normal(theta.size)).astype(np.float32)


def gnn_unpack(theta, k, f, num_layers, dtype=np.float64):
  out, off = [], 0
  th = np.asarray(theta, dtype)
  shapes = gnn_param_shapes(k, f, num_layers)
  for i in range(0, len(shapes), 2):
    nw, nb = int(np.prod(shapes[i])), int(np.prod(shapes[i + 1]))
    out.append((th[off:off + nw].reshape(shapes[i])[0], th[off + nw:off + nw + nb]))
    off += nw + nb
  assert off == th.size
  return out


# --------------------------------------------------------------------------- forward / backward
def gnn_forward(theta, configs, adj, f, num_layers, nonlinearity='relu', dtype=np.float64,
                return_tape=False):
  """The pre-output-activation scalar of GraphConvNetwork: reduce_sum of the last map."""
  adj = np.asarray(adj)
  k = adj.shape[1]
  a = np.asarray(configs, dtype)[:, :, None]                     # tf.expand_dims(inputs, 2)
  layers_ = gnn_unpack(theta, k, f, num_layers, dtype)
  act = vo.NONLINEARITIES[nonlinearity]
  tape = []
  for l, (w, b) in enumerate(layers_):
    z = np.einsum('bntc,tco->bno', a[:, adj], w, optimize=True) + b
    tape.append((a, z))
    a = act(z) if l + 1 != num_layers else z
  logit = a.reshape(a.shape[0], -1).sum(1)
  if return_tape == 'scale':
    return logit, np.abs(a).reshape(a.shape[0], -1).sum(1)
  if return_tape:
    return logit, tape, layers_
  return logit


def gnn_psi(theta, configs, adj, f, num_layers, shift=-10.0, nonlinearity='relu',
            output_activation='exp', dtype=np.float64):
  logit = gnn_forward(theta, configs, adj, f, num_layers, nonlinearity, dtype)
  if output_activation == 'exp':
    with np.errstate(over='ignore'):
      return np.exp(logit - dtype(shift))
  return vo.NONLINEARITIES[output_activation](logit)


def gnn_weighted_grads(theta, configs, weights, adj, f, num_layers, nonlinearity='relu',
                       output_activation='exp', dtype=np.float64):
  """sum_b weights[b, c] d log psi_b / d theta -> [C, P] (manual back-propagation; the transposed
  gather is a scatter-add over the table)."""
  adj = np.asarray(adj)
  w_b = np.asarray(weights, dtype)
  if w_b.ndim == 1:
    w_b = w_b[:, None]
  logit, tape, layers_ = gnn_forward(theta, configs, adj, f, num_layers, nonlinearity, dtype, True)
  w_b = w_b * vo.output_dlog(logit, output_activation, dtype)[:, None]
  dact = vo._NONLIN_DERIV[nonlinearity]
  out = []
  for c in range(w_b.shape[1]):
    grads = [None] * num_layers
    delta = np.broadcast_to(w_b[:, c][:, None, None], tape[-1][1].shape).astype(dtype)
    for l in range(num_layers - 1, -1, -1):
      a_in, _ = tape[l]
      xg = a_in[:, adj]                                          # [B, N, k, Cin]
      w, _ = layers_[l]
      grads[l] = (np.einsum('bntc,bno->tco', xg, delta, optimize=True)[None], delta.sum((0, 1)))
      if l > 0:
        dxg = np.einsum('bno,tco->bntc', delta, w, optimize=True)
        dx = np.zeros_like(a_in)
        for t in range(adj.shape[1]):
          np.add.at(dx, (slice(None), adj[:, t]), dxg[:, :, t])
        z_prev = tape[l - 1][1]
        delta = dx * dact(z_prev, vo.NONLINEARITIES[nonlinearity](z_prev))
    out.append(np.concatenate([np.concatenate([g[0].ravel(), g[1].ravel()]) for g in grads]))
  return np.stack(out)


def gnn_per_sample_grads(theta, configs, adj, f, num_layers, nonlinearity='relu', dtype=np.float64):
  """O[b, p] = d logit_b / d theta_p (small batches: one-hot weights)."""
  b = np.asarray(configs).shape[0]
  return gnn_weighted_grads(theta, configs, np.eye(b), adj, f, num_layers, nonlinearity, 'exp', dtype)


# --------------------------------------------------------------------------- accumulators
def energy_gradient_accumulate(acc, theta, configs, bonds, j_x, j_z, shift, adj, f, num_layers,
                               nonlinearity='relu', output_activation='exp'):
  """vo.energy_gradient_accumulate (training.py:539-558) on the gnn ansatz, in fp64."""
  amp = lambda c: gnn_psi(theta, c, adj, f, num_layers, shift, nonlinearity, output_activation)
  psi = amp(configs)
  e_loc = vo.local_value(amp, configs, bonds, j_x, j_z, psi, np.float64)
  g = gnn_weighted_grads(theta, configs, np.stack([np.ones_like(e_loc), e_loc], 1), adj, f,
                         num_layers, nonlinearity, output_activation)
  acc.g1_total += g[0]; acc.g2_total += g[1]; acc.g_count += 1
  acc.e_total += e_loc.sum(); acc.e_count += e_loc.size
  return e_loc


def log_overlap_accumulate(acc, theta, theta_omega, configs, bonds, j_x, j_z, shift, shift_omega,
                           beta, adj, f, num_layers, nonlinearity='relu', output_activation='exp'):
  """vo.log_overlap_accumulate (training.py:661-695) on the gnn ansatz, in fp64."""
  amp = lambda c: gnn_psi(theta, c, adj, f, num_layers, shift, nonlinearity, output_activation)
  amp_w = lambda c: gnn_psi(theta_omega, c, adj, f, num_layers, shift_omega, nonlinearity,
                            output_activation)
  psi = amp(configs)
  psi_w = amp_w(configs)
  h_psi_w = vo.apply_in_place(amp_w, configs, bonds, j_x, j_z, psi_w, np.float64)
  ratio = (psi_w - beta * h_psi_w) / psi
  e_loc = h_psi_w / psi_w
  g = gnn_weighted_grads(theta, configs, np.stack([np.ones_like(ratio), ratio], 1), adj, f,
                         num_layers, nonlinearity, output_activation)
  acc.g1_total += g[0]; acc.g2_total += g[1]; acc.g_count += 1
  acc.e_total += e_loc.sum(); acc.e_count += e_loc.size
  acc.r_total += ratio.sum(); acc.r_count += ratio.size
  return e_loc, ratio

"""Symmetry evaluation driver (extension: the reference has run_energy_evaluation only).

Reads `hparams.pbtxt` (+ optional `J.txt`) and the latest checkpoint of --checkpoint_dir as run_energy_evaluation
does, runs SymmetryEvaluator -- <P_g> = <psi(g x) / psi(x)> over the chains for site permutations g, optionally followed by
the global spin flip -- and writes into --output_dir (default: the checkpoint directory)
  symmetries.txt         label flip value err          one line per op, in the ops' order
  momentum_weights.txt   q... weight err               the weight of the state at each allowed momentum
The ops are those of --ops_file (one op per line: an optional leading word `flip`, then the site indices perm[0] perm[1]
...; the row of a configuration s is s[perm[i]]), or without a file the N translations of the lattice, then its
point-group elements without the identity, then -- with --spin_flip -- the global flip alone and every earlier op
followed by it.  The default ops need the lattice: hparams size_x * size_y = num_sites (the torus of lattice.torus_bonds:
site = x + size_x * y; set them with --hparams size_x=..,size_y=..) or the bonds of the periodic chain.  The second file
is written when the first N ops are the translations; its errors are the standard errors of the per-sample weights.
"""
from __future__ import annotations

import os

import numpy as np

from . import cli_common
from . import evaluation
from . import lattice
from . import run_correlation_evaluation

FLAG_TABLE = cli_common.measurement_flag_table((
    ('ops_file', str, '', 'Text file of ops, one per line: [flip] perm[0] perm[1] ... (default: the lattice\'s symmetries).'),
    ('spin_flip', bool, False, 'Without --ops_file: also the global spin flip, alone and after every other op.'),
), 'the two files go')


def lattice_sizes(hparams, bonds):
  """(size_x, size_y) of the lattice the run lives on (size_y = 1: the periodic chain), found as
  run_correlation_evaluation.lattice_geometry finds it, or None when it is not known."""
  geometry = run_correlation_evaluation.lattice_geometry(hparams, bonds)
  if geometry is None:
    return None
  if geometry[0].shape[1] == 1:
    return hparams.num_sites, 1
  return hparams.size_x, hparams.size_y


def default_ops(size_x: int, size_y: int, spin_flip: bool):
  """(labels, perms [n_ops][N] int32, flips [n_ops] uint8): the N translations (`T(r)` on a chain, `T(r_x,r_y)` on a
  torus), the point-group elements without the identity and, with spin_flip, `flip` and every earlier op + `+flip`."""
  n = size_x * size_y
  labels = ['T({})'.format(r) if size_y == 1 else 'T({},{})'.format(r % size_x, r // size_x) for r in range(n)]
  names, group = lattice.point_group(size_x, size_y)
  labels += names[1:]
  perms = np.concatenate([lattice.translations(size_x, size_y), group[1:]])
  flips = np.zeros(len(perms), np.uint8)
  if spin_flip:
    labels += ['flip'] + [name + '+flip' for name in labels[1:]]
    perms = np.concatenate([perms, perms])
    flips = np.concatenate([flips, np.ones_like(flips)])
  return labels, np.ascontiguousarray(perms), flips


def load_ops(path: str, spin_flip: bool, hparams, bonds):
  """(labels, perms, flips) of a file (lattice.read_symmetry_ops; labels `op0`, `op1`, ...), or the default ops of the
  lattice without one; validated against num_sites."""
  if path:
    perms, flips = lattice.read_symmetry_ops(path)
    lengths = {len(p) for p in perms}
    if lengths != {hparams.num_sites}:
      raise ValueError('{}: every op needs {} site indices'.format(path, hparams.num_sites))
    labels = ['op{}'.format(k) for k in range(len(perms))]
  else:
    sizes = lattice_sizes(hparams, bonds)
    if sizes is None:
      raise ValueError('the lattice is not known: give --ops_file, or --hparams size_x=..,size_y=.. with size_x * size_y = '
                       'num_sites')
    labels, perms, flips = default_ops(sizes[0], sizes[1], spin_flip)
  perms, flips = lattice.check_symmetry_ops(perms, flips, hparams.num_sites)
  return labels, perms, flips


def write_symmetries(directory: str, labels, result) -> str:
  path = os.path.join(directory, 'symmetries.txt')
  with open(path, 'w') as f:
    f.write('# label flip value err\n')
    for label, flip, value, err in zip(labels, result['flips'], result['value'], result['value_err']):
      f.write('{} {} {:.10g} {:.3g}\n'.format(label, int(flip), value, err))
  return path


def momentum_weights_of(result, size_x: int, size_y: int):
  """(weights [N], errors [N]) from the first N ops of `result` when they are the translations without a flip, else
  None: the weights of the mean values and the standard errors of the per-sample weights."""
  n = size_x * size_y
  perms, flips = result['perms'], result['flips']
  if len(perms) < n or flips[:n].any() or not np.array_equal(perms[:n], lattice.translations(size_x, size_y)):
    return None
  per_sample = lattice.momentum_weights(result['samples'][:, :n], size_x, size_y)
  return lattice.momentum_weights(result['value'][:n], size_x, size_y), evaluation._std_err(per_sample)


def write_momentum_weights(directory: str, qs, weights, errors) -> str:
  path = os.path.join(directory, 'momentum_weights.txt')
  with open(path, 'w') as f:
    f.write('# {} weight err\n'.format(' '.join('q' + 'xyz'[d] for d in range(qs.shape[1]))))
    for q, w, e in zip(qs, weights, errors):
      f.write('{} {:.10g} {:.3g}\n'.format(' '.join('{:.10g}'.format(x) for x in q), w, e))
  return path


def evaluate(flags):
  """-> (hparams, bonds, labels, result dict of SymmetryEvaluator.run_evaluation)."""
  labels = []

  def load_operator(hp, bonds):
    names, perms, flips = load_ops(flags.ops_file, flags.spin_flip, hp, bonds)
    labels.extend(names)
    return perms, flips
  hp, bonds, result = cli_common.evaluate_measurement(flags, evaluation.SymmetryEvaluator(), load_operator)
  return hp, bonds, labels, result


def write_files(out_dir: str, hp, bonds, labels, result):
  written = [write_symmetries(out_dir, labels, result)]
  sizes = lattice_sizes(hp, bonds)
  weights = momentum_weights_of(result, *sizes) if sizes is not None else None
  if weights is not None:
    qs = lattice.chain_momenta(sizes[0]) if sizes[1] == 1 else lattice.torus_momenta(*sizes)
    written.append(write_momentum_weights(out_dir, qs, *weights))
  return written


def main(argv=None):
  return cli_common.measurement_main(__doc__, FLAG_TABLE, argv, evaluate, write_files)


if __name__ == '__main__':
  main()

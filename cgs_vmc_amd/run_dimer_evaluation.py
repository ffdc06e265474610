"""Dimer-dimer correlation evaluation driver (extension: the reference has run_energy_evaluation only).

Reads `hparams.pbtxt` (+ optional `J.txt`) and the latest checkpoint of --checkpoint_dir as run_energy_evaluation
does, runs DimerCorrelationEvaluator and writes into --output_dir (default: the checkpoint directory)
  dimer_correlations.txt       i j k l dd dd_err connected connected_err      one line per pair of bonds, in the pairs' order
  dimer_structure_factor.txt   q... D_x(q) [D_y(q)]                           on the lattice's allowed momenta
with dd = <(S_i . S_j)(S_k . S_l)> and connected = dd - <S_i . S_j><S_k . S_l>.  The bonds are those of --bonds_file
(lattice.read_bond_pairs: lines `i j`; default: the Hamiltonian's, `J.txt` or the periodic chain), each paired with
bond number --reference_bond as (reference, bond); a bonds file with lines `i j k l` names the pairs itself.  The
second file needs positions: it is written when hparams size_x * size_y = num_sites (the torus of
lattice.torus_bonds: site = x + size_x * y; set them with --hparams size_x=..,size_y=..) or when the Hamiltonian's
bonds are the periodic chain.
"""
from __future__ import annotations

import os

import numpy as np

from . import cli_common
from . import evaluation
from . import lattice

FLAG_TABLE = cli_common.measurement_flag_table((
    ('bonds_file', str, '', 'Text file of bonds `i j` (or of pairs of bonds `i j k l`); default: the bonds of J.txt.'),
    ('reference_bond', int, 0, 'Index of the bond every bond of the list is paired with.'),
), 'the two files go')


def load_bond_pairs(path: str, reference_bond: int, hamiltonian_bonds, n_sites: int):
  """(bonds [n_bonds][2] int32, pairs [n_pairs][2] int32) of a run; validated against n_sites."""
  if path:
    bonds, pairs = lattice.read_bond_pairs(path)
  else:
    bonds, pairs = [[int(b[0]), int(b[1])] for b in hamiltonian_bonds], []
  if not bonds:
    raise ValueError('no bonds to measure')
  bonds = np.asarray(bonds, np.int32).reshape(-1, 2)
  if bonds.min() < 0 or bonds.max() >= n_sites:
    raise ValueError('a bond names a site out of range 0 .. {}'.format(n_sites - 1))
  if (bonds[:, 0] == bonds[:, 1]).any():
    raise ValueError('a bond joins a site with itself')
  if not pairs:
    if not 0 <= reference_bond < len(bonds):
      raise ValueError('--reference_bond {} outside 0 .. {}'.format(reference_bond, len(bonds) - 1))
    pairs = [[reference_bond, b] for b in range(len(bonds))]
  return np.ascontiguousarray(bonds), np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))


def lattice_sizes(hparams, bonds):
  """(size_x, size_y) of the lattice the run lives on (size_y = 1: the periodic chain), or None when it is not known."""
  n = hparams.num_sites
  if hparams.size_x * hparams.size_y == n and min(hparams.size_x, hparams.size_y) >= 1 and n > 1:
    return int(hparams.size_x), int(hparams.size_y)
  as_set = lambda bs: {(min(int(b[0]), int(b[1])), max(int(b[0]), int(b[1]))) for b in bs}
  if as_set(bonds) == as_set(lattice.chain_bonds(n)):
    return n, 1
  return None


def write_dimer_correlations(directory: str, result) -> str:
  path = os.path.join(directory, 'dimer_correlations.txt')
  bonds = result['bonds']
  with open(path, 'w') as f:
    f.write('# i j k l dd dd_err connected connected_err\n')
    for (a, b), dd, de, cn, ce in zip(result['pairs'], result['dd'], result['dd_err'], result['connected'],
                                      result['connected_err']):
      f.write('{} {} {} {} {:.10g} {:.3g} {:.10g} {:.3g}\n'.format(int(bonds[a][0]), int(bonds[a][1]), int(bonds[b][0]),
                                                                 int(bonds[b][1]), dd, de, cn, ce))
  return path


def write_dimer_structure_factor(directory: str, qs, d_q) -> str:
  path = os.path.join(directory, 'dimer_structure_factor.txt')
  with open(path, 'w') as f:
    f.write('# {} {}\n'.format(' '.join('q' + 'xyz'[d] for d in range(qs.shape[1])),
                               ' '.join('D_' + 'xyz'[d] + '(q)' for d in range(d_q.shape[0]))))
    for k, q in enumerate(qs):
      f.write('{} {}\n'.format(' '.join('{:.10g}'.format(x) for x in q), ' '.join('{:.10g}'.format(x) for x in d_q[:, k])))
  return path


def evaluate(flags):
  """-> (hparams, the Hamiltonian's bonds, result dict of DimerCorrelationEvaluator.run_evaluation)."""
  return cli_common.evaluate_measurement(
      flags, evaluation.DimerCorrelationEvaluator(),
      lambda hp, bonds: load_bond_pairs(flags.bonds_file, flags.reference_bond, bonds, hp.num_sites))


def write_files(out_dir: str, hp, bonds, result):
  written = [write_dimer_correlations(out_dir, result)]
  sizes = lattice_sizes(hp, bonds)
  if sizes is not None:
    qs, d_q = lattice.dimer_structure_factor(result['bonds'], result['pairs'], result['connected'], *sizes)
    written.append(write_dimer_structure_factor(out_dir, qs, d_q))
  return written


def main(argv=None):
  return cli_common.measurement_main(__doc__, FLAG_TABLE, argv, evaluate, write_files)


if __name__ == '__main__':
  main()

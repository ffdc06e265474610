"""Spin-correlation evaluation driver (extension: the reference has run_energy_evaluation only).

Reads `hparams.pbtxt` (+ optional `J.txt`) and the latest checkpoint of --checkpoint_dir as run_energy_evaluation
does, runs SpinCorrelationEvaluator over --pairs_file (lines `i j`; default: all N (N - 1) / 2 pairs) and writes
into --output_dir (default: the checkpoint directory)
  correlations.txt       i j szsz exchange ss err      <S_i . S_j> = szsz + exchange, err its standard error
  structure_factor.txt   q... S(q)                     on the lattice's allowed momenta
The second file needs positions: it is written when hparams size_x * size_y = num_sites (the torus of
lattice.torus_bonds: site = x + size_x * y; set them with --hparams size_x=..,size_y=..) or when the bonds are
the periodic chain, and when the pairs are all pairs.
"""
from __future__ import annotations

import os

import numpy as np

from . import cli_common
from . import evaluation
from . import lattice

FLAG_TABLE = cli_common.measurement_flag_table((
    ('pairs_file', str, '', 'Text file of site pairs, one `i j` per line (default: all pairs).'),
), 'the two files go')


def load_pairs(path: str, n_sites: int) -> np.ndarray:
  """[n_pairs][2] int32 from a file of integer pairs (extra columns ignored), or all pairs without one."""
  if not path:
    return lattice.all_pairs(n_sites)
  data = np.atleast_2d(np.genfromtxt(path, usecols=(0, 1)))
  return np.ascontiguousarray(data.astype(np.int32))


def lattice_geometry(hparams, bonds):
  """(coords [N][d], allowed momenta [N][d]) of the lattice the run lives on, or None when it is not known."""
  n = hparams.num_sites
  if hparams.size_x * hparams.size_y == n and min(hparams.size_x, hparams.size_y) >= 1 and n > 1:
    return (lattice.torus_coords(hparams.size_x, hparams.size_y), lattice.torus_momenta(hparams.size_x, hparams.size_y))
  as_set = lambda bs: {(min(int(b[0]), int(b[1])), max(int(b[0]), int(b[1]))) for b in bs}
  if as_set(bonds) == as_set(lattice.chain_bonds(n)):
    return lattice.chain_coords(n), lattice.chain_momenta(n)
  return None


def write_correlations(directory: str, result) -> str:
  path = os.path.join(directory, 'correlations.txt')
  with open(path, 'w') as f:
    f.write('# i j szsz exchange ss err\n')
    for (i, j), zz, ex, ss, err in zip(result['pairs'], result['szsz'], result['exchange'], result['ss'], result['ss_err']):
      f.write('{} {} {:.10g} {:.10g} {:.10g} {:.3g}\n'.format(int(i), int(j), zz, ex, ss, err))
  return path


def write_structure_factor(directory: str, qs, s_q) -> str:
  path = os.path.join(directory, 'structure_factor.txt')
  with open(path, 'w') as f:
    f.write('# {} S(q)\n'.format(' '.join('q' + 'xyz'[d] for d in range(qs.shape[1]))))
    for q, s in zip(qs, s_q):
      f.write('{} {:.10g}\n'.format(' '.join('{:.10g}'.format(x) for x in q), s))
  return path


def evaluate(flags):
  """-> (hparams, bonds, result dict of SpinCorrelationEvaluator.run_evaluation)."""
  return cli_common.evaluate_measurement(flags, evaluation.SpinCorrelationEvaluator(),
                                         lambda hp, bonds: load_pairs(flags.pairs_file, hp.num_sites))


def write_files(out_dir: str, hp, bonds, result):
  written = [write_correlations(out_dir, result)]
  geometry = lattice_geometry(hp, bonds)
  n = hp.num_sites
  pairs = result['pairs']
  every_pair = len({(min(i, j), max(i, j)) for i, j in pairs.tolist()}) == len(pairs) == n * (n - 1) // 2
  if geometry is not None and every_pair:
    coords, qs = geometry
    written.append(write_structure_factor(out_dir, qs, lattice.structure_factor(result['ss'], pairs, coords, qs)))
  return written


def main(argv=None):
  return cli_common.measurement_main(__doc__, FLAG_TABLE, argv, evaluate, write_files)


if __name__ == '__main__':
  main()

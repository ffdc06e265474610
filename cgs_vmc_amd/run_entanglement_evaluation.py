"""Entanglement-entropy evaluation driver (extension: the reference has run_energy_evaluation only).

Reads `hparams.pbtxt` (+ optional `J.txt`) and the latest checkpoint of --checkpoint_dir as run_energy_evaluation
does, runs RenyiEntropyEvaluator (the replica swap estimator of S2 = -ln Tr rho_A^2 over chain pairs) over the regions
of --regions_file (one region per line as site indices; default: the blocks [0, l), l = 1 .. N / 2) and writes into
--output_dir (default: the checkpoint directory)
  entanglement.txt       size purity purity_err s2 s2_err match_fraction      one line per region, in the regions' order
batch_size must be even (per rank, with sharded chains): chain c is paired with chain c + batch_size / 2.
"""
from __future__ import annotations

import os

from . import cli_common
from . import evaluation
from . import lattice

FLAG_TABLE = cli_common.measurement_flag_table((
    ('regions_file', str, '', 'Text file of regions, one per line as site indices (default: the blocks [0, l)).'),
), 'entanglement.txt goes')


def load_regions(path: str, n_sites: int):
  """The regions of a file (lattice.read_regions), or the blocks without one; validated against n_sites."""
  regions = lattice.read_regions(path) if path else lattice.block_regions(n_sites)
  lattice.region_masks(regions, n_sites)
  return regions


def write_entanglement(directory: str, result) -> str:
  path = os.path.join(directory, 'entanglement.txt')
  with open(path, 'w') as f:
    f.write('# size purity purity_err s2 s2_err match_fraction\n')
    for mask, p, pe, s2, se, mf in zip(result['regions'], result['purity'], result['purity_err'], result['s2'],
                                       result['s2_err'], result['match_fraction']):
      f.write('{} {:.10g} {:.3g} {:.10g} {:.3g} {:.6g}\n'.format(int(mask.sum()), p, pe, s2, se, mf))
  return path


def evaluate(flags):
  """-> (hparams, result dict of RenyiEntropyEvaluator.run_evaluation)."""
  hp, _, result = cli_common.evaluate_measurement(flags, evaluation.RenyiEntropyEvaluator(),
                                                  lambda hp, bonds: load_regions(flags.regions_file, hp.num_sites))
  return hp, result


def main(argv=None):
  return cli_common.measurement_main(__doc__, FLAG_TABLE, argv, evaluate,
                                     lambda out_dir, hp, result: [write_entanglement(out_dir, result)])


if __name__ == '__main__':
  main()

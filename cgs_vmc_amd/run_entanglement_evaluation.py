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
from . import parallel
from . import session as session_lib
from . import utils

FLAG_TABLE = (
    ('checkpoint_dir', str, '', 'Full path to the checkpoint directory.'),
    ('regions_file', str, '', 'Text file of regions, one per line as site indices (default: the blocks [0, l)).'),
    ('output_dir', str, '', 'Where entanglement.txt goes (default: the checkpoint directory).'),
    ('hparams', str, '', 'Comma-separated name=value overrides of the hyper-parameters.'),
)


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
  hp = utils.load_hparams(os.path.join(flags.checkpoint_dir, 'hparams.pbtxt'))
  hp.parse(flags.hparams)
  ansatz, _ = cli_common.heisenberg_system(hp, flags.checkpoint_dir, 1.0)
  regions = load_regions(flags.regions_file, hp.num_sites)
  evaluator = evaluation.RenyiEntropyEvaluator()
  eval_ops = evaluator.build_eval_ops(**cli_common.graph_kwargs(wavefunction=ansatz, operator=regions, hparams=hp))
  sess = session_lib.Session()
  sess.run(session_lib.global_variables_initializer())
  session_lib.Saver(ansatz.get_trainable_variables()).restore(
      sess, session_lib.latest_checkpoint(hp.checkpoint_dir))
  return hp, evaluator.run_evaluation(eval_ops, sess, hp, epoch_num=0)


def main(argv=None):
  flags = cli_common.parser_from_table(__doc__, FLAG_TABLE).parse_args(argv)
  parallel.init_from_env('nccl')
  _, result = evaluate(flags)
  written = []
  if parallel.rank() == 0:
    out_dir = flags.output_dir or flags.checkpoint_dir
    cli_common.ensure_directory(out_dir)
    written.append(write_entanglement(out_dir, result))
    for path in written:
      print('wrote {}'.format(path))
  return result, written


if __name__ == '__main__':
  main()

"""Energy evaluation of a symmetrized run (extension): run_energy_evaluation for psi_s = sum_k chi_s(k) psi(g_k .).

Reads `hparams.pbtxt` (+ optional `J.txt`) and the latest checkpoint of --checkpoint_dir -- the base's variables, as
run_symmetrized_training (or a plain run_training of the base type) wrote them --, the ops and the characters of the
sector from `sector_ops.txt` / `sector_characters.txt` in --sector_dir (default: the checkpoint directory), samples
|psi_s|^2, runs MonteCarloOperatorEvaluator and writes `energy` -- the mean and its standard error on one line -- into the
checkpoint directory.  Prints `Energy: <mean> +/- <standard error>`.
"""
from __future__ import annotations

import os

import numpy as np

from . import cli_common
from . import evaluation
from . import parallel
from . import run_symmetrized_training as rst
from . import session as session_lib
from . import utils

FLAG_TABLE = (
    ('heisenberg_jx', float, 1.0, 'Jx value in Heisenberg Hamiltonian.'),
    ('checkpoint_dir', str, '', 'Full path to the checkpoint directory.'),
    ('sector_dir', str, '', 'Directory of sector_ops.txt / sector_characters.txt (default: the checkpoint directory).'),
    ('hparams', str, '', 'Comma-separated name=value overrides of the hyper-parameters.'),
)


def evaluate(flags):
  """-> float64 [num_evaluation_samples] batch means of the local energy of psi_s."""
  if parallel.is_distributed():
    raise NotImplementedError('run_symmetrized_energy_evaluation runs on one rank: a symmetrized ctx has no sharded entries')
  hp = utils.load_hparams(os.path.join(flags.checkpoint_dir, 'hparams.pbtxt'))
  hp.parse(flags.hparams)
  sector = rst.read_sector(flags.sector_dir or flags.checkpoint_dir, hp.num_sites)
  ansatz, hamiltonian = rst.symmetrized_system(hp, flags.checkpoint_dir, flags.heisenberg_jx, *sector)
  evaluator = evaluation.MonteCarloOperatorEvaluator()
  eval_ops = evaluator.build_eval_ops(**cli_common.graph_kwargs(wavefunction=ansatz, operator=hamiltonian, hparams=hp))
  sess = session_lib.Session()
  sess.run(session_lib.global_variables_initializer())
  session_lib.Saver(ansatz.get_trainable_variables()).restore(sess, session_lib.latest_checkpoint(hp.checkpoint_dir))
  return np.asarray(evaluator.run_evaluation(eval_ops, sess, hp, epoch_num=0), np.float64)


def main(argv=None):
  flags = cli_common.parser_from_table(__doc__, FLAG_TABLE).parse_args(argv)
  parallel.init_from_env('nccl')
  samples = evaluate(flags)
  mean = float(samples.mean())
  error = float(samples.std(ddof=1) / np.sqrt(samples.size)) if samples.size > 1 else float('nan')
  with open(os.path.join(flags.checkpoint_dir, 'energy'), 'w') as out:
    out.write('{:.12g} {:.12g}\n'.format(mean, error))
  print('Energy: {} +/- {}'.format(mean, error))
  return mean, error


if __name__ == '__main__':
  main()

"""Overlap evaluation driver (extension: the reference has run_energy_evaluation only).

Reads `hparams.pbtxt` (+ optional `J.txt`) and the latest checkpoint of --checkpoint_dir as run_energy_evaluation does --
that is psi, the state the chains are drawn from -- and the latest checkpoint of --other_dir into a second, frozen state
phi of the same architecture (its variable names and shapes must be psi's; the first that is not raises ValueError).  Runs
OverlapEvaluator -- F = |<phi|psi>|^2 / (<psi|psi><phi|phi>) = <r>^2 / <r^2>, r = phi / psi over the chains -- and
writes into --output_dir (default: the checkpoint directory)
  overlap.txt   fidelity fidelity_err overlap_sign alive_fraction      one line
overlap_sign is the sign of <phi|psi>; alive_fraction the share of chains whose own amplitude does not vanish.  One rank
only.
"""
from __future__ import annotations

import copy
import os

from . import cli_common
from . import evaluation
from . import session as session_lib
from . import training
from . import utils

FLAG_TABLE = cli_common.measurement_flag_table((
    ('other_dir', str, '', 'Run directory of the second state phi (its latest checkpoint is loaded).'),
), '`overlap.txt` goes')

OVERLAP_COLUMNS = ('fidelity', 'fidelity_err', 'overlap_sign', 'alive_fraction')


def write_overlap(directory: str, result) -> str:
  path = os.path.join(directory, 'overlap.txt')
  with open(path, 'w') as f:
    f.write('# {}\n'.format(' '.join(OVERLAP_COLUMNS)))
    f.write('{:.17g} {:.6g} {:.0f} {:.17g}\n'.format(*(result[k] for k in OVERLAP_COLUMNS)))
  return path


def read_overlap(directory: str):
  """{column: value} of an `overlap.txt`."""
  with open(os.path.join(directory, 'overlap.txt')) as f:
    rows = [line.split() for line in f if line.strip() and not line.startswith('#')]
  return dict(zip(OVERLAP_COLUMNS, (float(v) for v in rows[0])))


def evaluate(flags):
  """-> (hparams, result dict of OverlapEvaluator.run_evaluation)."""
  if not flags.other_dir:
    raise ValueError('--other_dir is required: the run directory of the second state')
  hp = utils.load_hparams(os.path.join(flags.checkpoint_dir, 'hparams.pbtxt'))
  hp.parse(flags.hparams)
  ansatz, _ = cli_common.heisenberg_system(hp, flags.checkpoint_dir, 1.0)
  other = copy.deepcopy(ansatz)
  evaluator = evaluation.OverlapEvaluator()
  eval_ops = evaluator.build_eval_ops(**cli_common.graph_kwargs(wavefunction=ansatz, operator=other, hparams=hp))
  sess = session_lib.Session()
  sess.run(session_lib.global_variables_initializer())
  session_lib.Saver(ansatz.get_trainable_variables()).restore(sess, session_lib.latest_checkpoint(hp.checkpoint_dir))
  training.load_frozen_state(ansatz, other, flags.other_dir)
  return hp, evaluator.run_evaluation(eval_ops, sess, hp, epoch_num=0)


def write_files(out_dir: str, hp, result):
  del hp
  return [write_overlap(out_dir, result)]


def main(argv=None):
  return cli_common.measurement_main(__doc__, FLAG_TABLE, argv, evaluate, write_files)


if __name__ == '__main__':
  main()

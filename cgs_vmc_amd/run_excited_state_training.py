"""Excited-state optimisation driver (extension: the reference trains ground states only).

Trains E[psi] + overlap_penalty * F(psi, phi) against a frozen lower state phi of the same architecture (Choo et al.
2018): with the penalty above the gap, the minimum is the first excited state of the sampled sector.  The flags are
run_training's plus
  --lower_state_dir   run directory of the lower state: its latest checkpoint is loaded into phi.  Its variable names
                      and shapes must be psi's; the first that is not raises ValueError.
  --overlap_penalty   the penalty (> 0), in units of the energy.
and --optimizer names a key of training.EXCITED_STATE_OPTIMIZERS.  Like run_training it writes `hparams.pbtxt`, one
checkpoint `model_prior_{epoch}_epochs` BEFORE every epoch (5 kept) and one energy per line appended to `metrics.txt`;
beside them one fidelity per line -- the epoch's mean of the batch estimates S1^2 / (alive S2) -- appended to
`overlap_metrics.txt`.  One rank only.

  python -m cgs_vmc_amd.run_excited_state_training --checkpoint_dir=/tmp/excited --lower_state_dir=/tmp/ground \\
      --overlap_penalty=2.0 --num_sites=16 --wavefunction_type=fully_connected --num_epochs=10 \\
      --heisenberg_jx=-1.0 --hparams="batch_size=64,fc_layer_size=32,num_fc_layers=2"
"""
from __future__ import annotations

import os
import sys

from . import cli_common
from . import parallel
from . import run_training
from . import session as session_lib
from . import training

FLAG_TABLE = tuple(
    ('optimizer', str, 'PenalizedEnergyGradient', 'Key of training.EXCITED_STATE_OPTIMIZERS.') if row[0] == 'optimizer' else row
    for row in run_training.FLAG_TABLE) + (
        ('lower_state_dir', str, '', 'Run directory of the frozen lower state (its latest checkpoint is loaded).'),
        ('overlap_penalty', float, 0.0, 'Penalty on the fidelity with the lower state (> 0), in units of the energy.'),
    )


def check_lower_state(ansatz, num_sites: int, directory: str):
  """training.check_lower_state for `ansatz` before it is connected to an engine: the latest checkpoint of `directory`
  must hold every variable of `ansatz` on `num_sites` sites, name and shape."""
  if getattr(ansatz, '_n_sites', None) is None:
    ansatz._n_sites = int(num_sites)
  return training.check_lower_state(ansatz.get_trainable_variables(), directory)


def write_overlap_metric(run_dir: str, fidelity: float) -> str:
  path = os.path.join(run_dir, 'overlap_metrics.txt')
  with open(path, 'a') as out:
    out.write('{}\n'.format(fidelity))
  return path


def read_overlap_metrics(run_dir: str):
  with open(os.path.join(run_dir, 'overlap_metrics.txt')) as f:
    return [float(line) for line in f if line.strip()]


def train(flags, hp):
  run_dir = hp.checkpoint_dir
  ansatz, hamiltonian = cli_common.heisenberg_system(hp, flags.checkpoint_dir, flags.heisenberg_jx,
                                                     getattr(flags, 'four_spin_q', 1.0))
  check_lower_state(ansatz, hp.num_sites, flags.lower_state_dir)     # before an engine is asked for
  optimizer = training.EXCITED_STATE_OPTIMIZERS[flags.optimizer]()
  train_ops = optimizer.build_opt_ops(**cli_common.graph_kwargs(
      wavefunction=ansatz, hamiltonian=hamiltonian, hparams=hp))

  sess = session_lib.Session()
  sess.run([session_lib.global_variables_initializer(),
            session_lib.local_variables_initializer()])

  saver = session_lib.Saver(ansatz.get_trainable_variables(), max_to_keep=5)
  if flags.resume_training:
    saver.restore(sess, session_lib.latest_checkpoint(run_dir))

  metrics_path = os.path.join(run_dir, 'metrics.txt')
  for epoch in range(flags.num_epochs):
    saver.save(sess, os.path.join(run_dir, 'model_prior_{}_epochs'.format(epoch)))   # the parameters PRIOR to this epoch
    energy = optimizer.run_optimization_epoch(train_ops, sess, hp)
    with open(metrics_path, 'a') as out:
      out.write('{}\n'.format(energy))
    write_overlap_metric(run_dir, optimizer.last_fidelity)
  return sess


def main(argv=None):
  flags = cli_common.parser_from_table(__doc__, FLAG_TABLE + cli_common.FOUR_SPIN_FLAGS).parse_args(argv)
  if flags.optimizer not in training.EXCITED_STATE_OPTIMIZERS:
    raise ValueError('--optimizer {!r} is no key of training.EXCITED_STATE_OPTIMIZERS {}'.format(
        flags.optimizer, sorted(training.EXCITED_STATE_OPTIMIZERS)))
  if not flags.lower_state_dir:
    raise ValueError('--lower_state_dir is required: the run directory of the frozen lower state')
  if not flags.overlap_penalty > 0:
    raise ValueError('--overlap_penalty must be > 0, got {}'.format(flags.overlap_penalty))
  parallel.init_from_env('nccl')
  if parallel.is_distributed():
    raise NotImplementedError('run_excited_state_training runs on one rank')
  hp = run_training.hparams_from_flags(flags)
  cli_common.ensure_directory(flags.checkpoint_dir)
  pbtxt = os.path.join(hp.checkpoint_dir, 'hparams.pbtxt')
  if os.path.exists(pbtxt) and not flags.override:
    print('Hparams file already exists')
    sys.exit()
  with open(pbtxt, 'w') as out:
    out.write(str(hp.to_proto()))
  # not hyper-parameters of the ansatz: they stay out of hparams.pbtxt, which the evaluation drivers read back
  hp.overlap_penalty = float(flags.overlap_penalty)
  hp.lower_state_dir = flags.lower_state_dir
  train(flags, hp)
  if flags.generate_vectors:
    raise NotImplementedError('--generate_vectors (VectorWavefunctionEvaluator) is outside '
                              'the MI355X hot path')


if __name__ == '__main__':
  main()

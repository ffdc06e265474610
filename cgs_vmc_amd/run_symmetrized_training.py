"""Training inside one symmetry sector (extension: the reference has run_training only).

Optimises the projected state itself, psi_s(x) = sum_k chi_s(k) psi(g_k x): the chains are sampled from |psi_s|^2 and
the parameters of psi follow the energy gradient of psi_s (wavefunctions.SymmetrizedWavefunction, vmc_create_symmetrized).
From the ground state's sector this gives a lower variational energy; from any other sector its lowest state as a
ground-state problem of its own.

  python -m cgs_vmc_amd.run_symmetrized_training --checkpoint_dir=/tmp/run --num_sites=8 --sector=q4 \\
      --wavefunction_type=fully_connected --num_epochs=100 --hparams="batch_size=64,fc_layer_size=32,num_fc_layers=2"

Takes run_training's flags (--optimizer is EnergyGradient and nothing else) plus the sector: --ops_file / --characters_file
(run_projected_energy_evaluation's formats; both or neither) or without files the N translations of the lattice -- the
periodic chain, or hparams size_x x size_y -- with --spin_flip followed by the same translations after the global spin
flip, and the characters of lattice.sector_characters; --sector names the row (`q4` on the 8-site chain is k = pi, `q2,2` on
the 4 x 4 torus (pi, pi), `q0-` the flip-odd sector at k = 0).  Every op must map the bonds onto themselves.
Writes `hparams.pbtxt`, `metrics.txt` and the checkpoints as run_training does -- the variables are the base's, under the
base's names: run_energy_evaluation, run_projected_energy_evaluation and run_training --resume_training read them as a
plain run's -- and `sector_ops.txt` / `sector_characters.txt` (the one chosen row) for
run_symmetrized_energy_evaluation.  The sector is no hyper-parameter: it stays out of hparams.pbtxt.
"""
from __future__ import annotations

import os

import numpy as np

from . import cli_common
from . import lattice
from . import operators
from . import parallel
from . import run_projected_energy_evaluation as rpe
from . import run_training
from . import session as session_lib
from . import training
from . import wavefunctions

OPS_FILE, CHARACTERS_FILE = 'sector_ops.txt', 'sector_characters.txt'

FLAG_TABLE = tuple(
    ('optimizer', str, 'EnergyGradient', 'EnergyGradient: the only optimizer with a symmetrized form.') if row[0] == 'optimizer'
    else row for row in run_training.FLAG_TABLE) + (
    ('ops_file', str, '', 'Text file of ops, one per line: [flip] perm[0] perm[1] ... (default: the translations).'),
    ('characters_file', str, '', 'Text file of characters, one sector per line: label chi[0] chi[1] ... (with --ops_file).'),
    ('sector', str, '', 'Label of the sector to train in (a row of the characters).'),
    ('spin_flip', bool, False, 'Without --ops_file: also every translation followed by the global spin flip.'),
)


def choose_sector(flags, hparams, bonds):
  """(label, perms, flips, chi [n_ops]) of --sector among the sectors of the files or of the lattice."""
  labels, perms, flips, chi = rpe.load_sectors(flags.ops_file, flags.characters_file, flags.spin_flip, hparams, bonds)
  if flags.sector not in labels:
    raise ValueError('--sector {!r} is none of the sectors {}'.format(flags.sector, ', '.join(labels)))
  return flags.sector, perms, flips, chi[labels.index(flags.sector)]


def write_sector(directory: str, label: str, perms, flips, chi):
  lattice.write_symmetry_ops(os.path.join(directory, OPS_FILE), perms, flips)
  lattice.write_characters(os.path.join(directory, CHARACTERS_FILE), [label], np.asarray(chi, np.float64)[None, :])


def read_sector(directory: str, num_sites: int):
  """(label, perms, flips, chi [n_ops]) as write_sector wrote them."""
  perms, flips = lattice.read_symmetry_ops(os.path.join(directory, OPS_FILE))
  perms, flips = lattice.check_symmetry_ops(perms, flips, num_sites)
  labels, chi = lattice.read_characters(os.path.join(directory, CHARACTERS_FILE))
  chi = lattice.check_characters(chi, len(perms))
  if len(labels) != 1:
    raise ValueError('{}: one sector expected, found {}'.format(os.path.join(directory, CHARACTERS_FILE), len(labels)))
  return labels[0], perms, flips, chi[0]


def symmetrized_system(hparams, directory: str, j_x: float, label, perms, flips, chi):
  """(symmetrized ansatz, Hamiltonian): cli_common.heisenberg_system with the base wrapped."""
  del label
  cli_common.refuse_four_spin_terms(directory, 'the symmetrized drivers', 'a symmetrized ctx takes no four-spin terms')
  base, hamiltonian = cli_common.heisenberg_system(hparams, directory, j_x)
  lattice.check_hamiltonian_symmetry(hamiltonian._bonds_list, j_x, 1.0, perms)
  return wavefunctions.SymmetrizedWavefunction(base, perms, flips if np.any(flips) else None, chi), hamiltonian


def train(flags, hp):
  if flags.optimizer != 'EnergyGradient':
    raise NotImplementedError('run_symmetrized_training: only --optimizer EnergyGradient is available on a symmetrized '
                              'wavefunction (got {!r})'.format(flags.optimizer))
  if parallel.is_distributed():
    raise NotImplementedError('run_symmetrized_training runs on one rank: a symmetrized ctx has no sharded entries')
  run_dir = hp.checkpoint_dir
  bonds = lattice.load_bonds(flags.checkpoint_dir, hp.num_sites)
  sector = choose_sector(flags, hp, bonds)
  ansatz, hamiltonian = symmetrized_system(hp, flags.checkpoint_dir, flags.heisenberg_jx, *sector)
  write_sector(run_dir, *sector)
  optimizer = training.GROUND_STATE_OPTIMIZERS[flags.optimizer]()
  train_ops = optimizer.build_opt_ops(**cli_common.graph_kwargs(wavefunction=ansatz, hamiltonian=hamiltonian, hparams=hp))
  sess = session_lib.Session()
  sess.run([session_lib.global_variables_initializer(), session_lib.local_variables_initializer()])
  saver = session_lib.Saver(ansatz.get_trainable_variables(), max_to_keep=5)
  if flags.resume_training:
    saver.restore(sess, session_lib.latest_checkpoint(run_dir))
  metrics_path = os.path.join(run_dir, 'metrics.txt')
  for epoch in range(flags.num_epochs):
    saver.save(sess, os.path.join(run_dir, 'model_prior_{}_epochs'.format(epoch)))     # the parameters PRIOR to this epoch
    energy = optimizer.run_optimization_epoch(train_ops, sess, hp)
    with open(metrics_path, 'a') as out:
      out.write('{}\n'.format(energy))
  return sess


def main(argv=None):
  flags = cli_common.parser_from_table(__doc__, FLAG_TABLE).parse_args(argv)
  parallel.init_from_env('nccl')
  hp = run_training.hparams_from_flags(flags)
  cli_common.ensure_directory(flags.checkpoint_dir)
  pbtxt = os.path.join(hp.checkpoint_dir, 'hparams.pbtxt')
  if os.path.exists(pbtxt) and not flags.override:
    print('Hparams file already exists')
    return None
  with open(pbtxt, 'w') as out:
    out.write(str(hp.to_proto()))
  return train(flags, hp)


if __name__ == '__main__':
  main()

"""Shared plumbing of the command-line drivers (flag tables, system construction,
parameter broadcast, the skeleton of the measurement drivers).  The drivers keep the reference's command-line contract
(cgs_vmc/run_training.py:21-68, run_energy_evaluation.py:19-37) but are organised around
these helpers instead of one long main()."""
from __future__ import annotations

import argparse
import os
from typing import Dict, Sequence, Tuple

from . import lattice
from . import operators
from . import parallel
from . import session as session_lib
from . import utils
from . import wavefunctions


def _flag_bool(text) -> bool:
  return str(text).strip().lower() in ('1', 'true', 't', 'yes', 'y')


# The flag of the drivers that train or evaluate the Hamiltonian of a run directory (run_training, run_energy_evaluation,
# run_excited_state_training): their parsers take it beside their FLAG_TABLE, which keeps the reference's command-line
# contract.  No other driver has it.
FOUR_SPIN_FLAGS = (
    ('four_spin_q', float, 1.0, 'Coupling q of the rows of `Q.txt` (four-spin terms) that state none.'),
)


def parser_from_table(description: str, table: Sequence[Tuple[str, type, object, str]]
                      ) -> argparse.ArgumentParser:
  """Builds an absl-like parser: --name=value or --name value; booleans also bare."""
  ap = argparse.ArgumentParser(description=description,
                               formatter_class=argparse.RawTextHelpFormatter)
  for name, kind, default, text in table:
    if kind is bool:
      ap.add_argument('--' + name, type=_flag_bool, nargs='?', const=True, default=default,
                      help=text)
    else:
      ap.add_argument('--' + name, type=kind, default=default, help=text)
  return ap


def heisenberg_system(hparams, directory: str, j_x: float, four_spin_q: float = 1.0):
  """(ansatz, Hamiltonian) for a run directory: the bond list comes from `J.txt` when the
  directory has one, otherwise the periodic chain of hparams.num_sites sites; j_z is fixed to 1
  as in the reference (run_training.py:112-113).  A directory that holds `Q.txt` (rows `i j k l [q]`,
  lattice.read_four_spin_terms) gets the operators.JQHamiltonian of the bonds and those four-spin terms -- rows without a
  fifth column take four_spin_q (--four_spin_q), the exchange sign is the sign of j_x; without the file nothing changes."""
  bonds = lattice.load_bonds(directory, hparams.num_sites)
  ansatz = wavefunctions.build_wavefunction(hparams)
  four_spin = lattice.load_four_spin_terms(directory, four_spin_q)
  if four_spin is not None:
    return ansatz, operators.JQHamiltonian(bonds, j_x, 1., four_spin[0], four_spin[1])
  return ansatz, operators.HeisenbergHamiltonian(bonds, j_x, 1.)


def refuse_four_spin_terms(directory: str, driver: str, why: str):
  """NotImplementedError when the run directory holds `Q.txt`: `driver` would silently leave the four-spin terms out."""
  if os.path.exists(os.path.join(directory, 'Q.txt')):
    raise NotImplementedError('{}: {} holds Q.txt (four-spin terms), and {}'.format(driver, directory, why))


def broadcast_parameters(ansatz):
  """All ranks start from rank 0's freshly initialised parameters."""
  if parallel.world_size() == 1:
    return
  theta = ansatz._get_theta()
  mine = theta if parallel.rank() == 0 else 0.0 * theta
  ansatz._set_theta(parallel.allreduce_array(mine).astype('float32'))


def ensure_directory(path: str):
  if path and not os.path.isdir(path):
    os.makedirs(path, exist_ok=True)


def graph_kwargs(**parts) -> Dict[str, object]:
  """Keyword bundle for build_opt_ops / build_eval_ops (they are called with keywords in the
  reference, run_training.py:120-127)."""
  parts.setdefault('shared_resources', {})
  return parts


def measurement_flag_table(own_rows, outputs: str):
  """The flag table of a measurement driver (run_correlation_evaluation, run_entanglement_evaluation,
  run_dimer_evaluation, run_symmetry_evaluation, run_projected_energy_evaluation, run_lanczos_evaluation, run_overlap_evaluation): --checkpoint_dir, the driver's own rows, --output_dir for `outputs`, --hparams."""
  return (('checkpoint_dir', str, '', 'Full path to the checkpoint directory.'),) + tuple(own_rows) + (
      ('output_dir', str, '', 'Where {} (default: the checkpoint directory).'.format(outputs)),
      ('hparams', str, '', 'Comma-separated name=value overrides of the hyper-parameters.'),
  )


def evaluate_measurement(flags, evaluator, load_operator):
  """A measurement driver's evaluation: `hparams.pbtxt` with the --hparams overrides, the Heisenberg system of the
  checkpoint directory, operator = load_operator(hparams, the Hamiltonian's bonds), the latest checkpoint restored.
  (Of the Hamiltonian the measurements of the state take the bond list alone: a `Q.txt` in the directory changes none of
  them.  The two that measure the Hamiltonian itself, run_lanczos_evaluation and run_projected_energy_evaluation, refuse
  such a directory: refuse_four_spin_terms.)
  -> (hparams, the Hamiltonian's bonds, the result of evaluator.run_evaluation)."""
  hp = utils.load_hparams(os.path.join(flags.checkpoint_dir, 'hparams.pbtxt'))
  hp.parse(flags.hparams)
  ansatz, hamiltonian = heisenberg_system(hp, flags.checkpoint_dir, 1.0)
  operator = load_operator(hp, hamiltonian._bonds_list)
  eval_ops = evaluator.build_eval_ops(**graph_kwargs(wavefunction=ansatz, operator=operator, hparams=hp))
  sess = session_lib.Session()
  sess.run(session_lib.global_variables_initializer())
  session_lib.Saver(ansatz.get_trainable_variables()).restore(
      sess, session_lib.latest_checkpoint(hp.checkpoint_dir))
  return hp, hamiltonian._bonds_list, evaluator.run_evaluation(eval_ops, sess, hp, epoch_num=0)


def measurement_main(doc: str, table, argv, evaluate, write):
  """main() of a measurement driver: evaluate(flags) -> (..., result) on every rank; rank 0 alone writes
  write(output directory, ..., result) -> paths, and prints them.  -> (result, paths written)."""
  flags = parser_from_table(doc, table).parse_args(argv)
  parallel.init_from_env('nccl')
  evaluated = evaluate(flags)
  result = evaluated[-1]
  written = []
  if parallel.rank() == 0:
    out_dir = flags.output_dir or flags.checkpoint_dir
    ensure_directory(out_dir)
    written = write(out_dir, *evaluated)
    for path in written:
      print('wrote {}'.format(path))
  return result, written

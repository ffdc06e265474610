"""Lanczos-step evaluation driver (extension: the reference has run_energy_evaluation only).

Reads `hparams.pbtxt` (+ optional `J.txt`) and the latest checkpoint of --checkpoint_dir as run_energy_evaluation does,
runs LanczosStepEvaluator -- the local values of H and H^2 per chain, the moments <H^n>, n = 1 .. 4, the best energy of
psi + alpha H psi, its variance and the energy extrapolated to zero variance through the two points -- and writes into
--output_dir (default: the checkpoint directory)
  lanczos.txt    name value error      one line per quantity of evaluation.LANCZOS_QUANTITIES
with the delete-one-sample jackknife error of each.  `h2_check` = <g> against `h2` = <e^2> is a sampling diagnostic: the
two estimate the same <H^2> and part company near nodes of a signed state.  j_x = --j_x (default 1), j_z = 1.
"""
from __future__ import annotations

import os

from . import cli_common
from . import evaluation
from . import operators

FLAG_TABLE = cli_common.measurement_flag_table((
    ('j_x', float, 1.0, 'The exchange coupling j_x of every bond (j_z = 1).'),
), 'lanczos.txt goes')


def write_lanczos(directory: str, result) -> str:
  path = os.path.join(directory, 'lanczos.txt')
  with open(path, 'w') as f:
    f.write('# name value error (delete-one-sample jackknife over {} samples)\n'.format(len(result['samples'])))
    for name in evaluation.LANCZOS_QUANTITIES:
      f.write('{} {!r} {!r}\n'.format(name, float(result[name]), float(result[name + '_err'])))
  return path


def read_lanczos(path: str):
  """{name: (value, error)} of a lanczos.txt."""
  out = {}
  with open(path) as f:
    for line in f:
      if line.startswith('#') or not line.strip():
        continue
      name, value, err = line.split()
      out[name] = (float(value), float(err))
  return out


def evaluate(flags):
  """-> (hparams, bonds, result dict of LanczosStepEvaluator.run_evaluation)."""
  cli_common.refuse_four_spin_terms(flags.checkpoint_dir, 'run_lanczos_evaluation',
                                    'the local values of H^2 do not cover them (vmc_energy_moments)')
  return cli_common.evaluate_measurement(
      flags, evaluation.LanczosStepEvaluator(), lambda hp, bonds: operators.HeisenbergHamiltonian(bonds, flags.j_x, 1.))


def write_files(out_dir: str, hp, bonds, result):
  del hp, bonds
  return [write_lanczos(out_dir, result)]


def main(argv=None):
  return cli_common.measurement_main(__doc__, FLAG_TABLE, argv, evaluate, write_files)


if __name__ == '__main__':
  main()

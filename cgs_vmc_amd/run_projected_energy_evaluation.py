"""Symmetry-projected energy evaluation driver (extension: the reference has run_energy_evaluation only).

Reads `hparams.pbtxt` (+ optional `J.txt`) and the latest checkpoint of --checkpoint_dir as run_energy_evaluation
does, runs ProjectedEnergyEvaluator -- E_s = <E_loc w_s> / <w_s>, w_s(x) = sum_k chi_s(k) psi(g_k x) / psi(x): the energy of
the state projected onto symmetry sector s, from chains sampled from |psi|^2 -- and writes into --output_dir (default: the
checkpoint directory)
  sector_energies.txt    label weight weight_err energy energy_err [unresolved]     one line per sector
with `unresolved` where |weight| < 3 weight_err: the state has no weight in that sector that the samples can tell from 0,
and the energy of the line is noise.  A last comment line gives the unprojected energy.
The ops are those of --ops_file (run_symmetry_evaluation's format) with the characters of --characters_file (one row
per sector: a label, then one real character per op; lattice.write_characters) -- both or neither -- or without files the
N translations of the lattice, with --spin_flip followed by the same translations after the global spin flip, and the
characters of lattice.sector_characters: one sector per momentum class {k, -k} (and parity).  The default ops need the
lattice: hparams size_x * size_y = num_sites (set them with --hparams size_x=..,size_y=..) or the bonds of the periodic
chain.  Every op must be a symmetry of the Hamiltonian (the library refuses anything else); j_x = j_z = 1 as in
run_symmetry_evaluation.
"""
from __future__ import annotations

import os

import numpy as np

from . import cli_common
from . import evaluation
from . import lattice
from . import operators
from . import run_symmetry_evaluation

FLAG_TABLE = cli_common.measurement_flag_table((
    ('ops_file', str, '', 'Text file of ops, one per line: [flip] perm[0] perm[1] ... (default: the translations).'),
    ('characters_file', str, '', 'Text file of characters, one sector per line: label chi[0] chi[1] ... (with --ops_file).'),
    ('spin_flip', bool, False, 'Without --ops_file: also every translation followed by the global spin flip.'),
), 'sector_energies.txt goes')


def load_sectors(ops_file: str, characters_file: str, spin_flip: bool, hparams, bonds):
  """(labels, perms, flips, chi) of the two files, or the translations and the sectors of the lattice without them."""
  if bool(ops_file) != bool(characters_file):
    raise ValueError('--ops_file and --characters_file go together: the characters are per op of the file')
  if ops_file:
    perms, flips = lattice.read_symmetry_ops(ops_file)
    if {len(p) for p in perms} != {hparams.num_sites}:
      raise ValueError('{}: every op needs {} site indices'.format(ops_file, hparams.num_sites))
    labels, chi = lattice.read_characters(characters_file)
  else:
    sizes = run_symmetry_evaluation.lattice_sizes(hparams, bonds)
    if sizes is None:
      raise ValueError('the lattice is not known: give --ops_file and --characters_file, or --hparams size_x=..,size_y=.. '
                       'with size_x * size_y = num_sites')
    t = lattice.translations(*sizes)
    perms = np.concatenate([t, t]) if spin_flip else t
    flips = np.repeat([0, 1], len(t)).astype(np.uint8) if spin_flip else np.zeros(len(t), np.uint8)
    labels, chi = lattice.sector_characters(sizes[0], sizes[1], spin_flip)
  perms, flips = lattice.check_symmetry_ops(perms, flips, hparams.num_sites)
  return labels, perms, flips, lattice.check_characters(chi, len(perms))


def unresolved(result):
  """[n_sectors] bool: |weight| < 3 weight_err."""
  return np.abs(result['weight']) < 3.0 * result['weight_err']


def write_sector_energies(directory: str, labels, result) -> str:
  path = os.path.join(directory, 'sector_energies.txt')
  with open(path, 'w') as f:
    f.write('# label weight weight_err energy energy_err [unresolved: |weight| < 3 weight_err]\n')
    for label, w, we, e, ee, flag in zip(labels, result['weight'], result['weight_err'], result['energy'],
                                         result['energy_err'], unresolved(result)):
      f.write('{} {:.12g} {:.12g} {:.12g} {:.12g}{}\n'.format(label, w, we, e, ee, ' unresolved' if flag else ''))
    f.write('# unprojected energy {:.12g} {:.12g}\n'.format(result['plain_energy'], result['plain_energy_err']))
  return path


def evaluate(flags):
  """-> (hparams, bonds, labels, result dict of ProjectedEnergyEvaluator.run_evaluation)."""
  labels = []

  def load_operator(hp, bonds):
    names, perms, flips, chi = load_sectors(flags.ops_file, flags.characters_file, flags.spin_flip, hp, bonds)
    labels.extend(names)
    return operators.HeisenbergHamiltonian(bonds, 1.0, 1.), perms, flips, chi
  cli_common.refuse_four_spin_terms(flags.checkpoint_dir, 'run_projected_energy_evaluation',
                                    'the symmetry check of the sector estimator does not cover them (vmc_projected_energy)')
  hp, bonds, result = cli_common.evaluate_measurement(flags, evaluation.ProjectedEnergyEvaluator(), load_operator)
  return hp, bonds, labels, result


def write_files(out_dir: str, hp, bonds, labels, result):
  del hp, bonds
  return [write_sector_energies(out_dir, labels, result)]


def main(argv=None):
  return cli_common.measurement_main(__doc__, FLAG_TABLE, argv, evaluate, write_files)


if __name__ == '__main__':
  main()

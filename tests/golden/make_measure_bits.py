"""Records tests/golden/measure_bits.npz: what the three measurements (vmc_pair_correlations, vmc_renyi2_swap,
vmc_dimer_correlations) return, bit for bit, on small fixed problems.  tests/test_gpu_measure_bits.py compares a build
against it with assert_array_equal.

PROVENANCE: like tail_bits.npz these vectors are NOT oracle outputs.  They are the results of the library itself on
an MI355X, recorded at the commit before the three C entries were merged into csrc/vmc_api_measure.hip (their host
scaffold, planner and device-buffer bookkeeping shared; no kernel's arithmetic touched).  Every value is an fp64 sum
folded in a fixed order, so they pin that order and the pass / buffer bookkeeping around it, not the physics (which
tests/test_gpu_corr.py, test_gpu_renyi.py and test_gpu_dimer.py check against the oracles).  Re-record only when a
change of the bits is intended:

  python tests/golden/make_measure_bits.py        # needs the GPU; rewrites tests/golden/measure_bits.npz

N = 16 on the 4 x 4 torus, B = 40 fixed chains (set_configs, no sampling), one ctx per family.  Per family the file
holds `<family>/<stage>/<quantity>`:
  eloc_before, eloc_after / eloc, diag, off     local_energy() and local_energy_terms() under the torus Hamiltonian
  corr_<tag> / zz, ex                           pair_correlations
  renyi_<tag> / swap, match                     renyi2_swap
  dimer_<tag> / bond, dd                        dimer_correlations
with <tag> = first3 (3 items on the fresh ctx: the buffers are allocated), full (the whole list, library's pass size:
they grow), again3 (3 items: they are larger than needed) and per<k> (the whole list at k items per pass).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, 'measure_bits.npz')
# fully_connected H = 32: unsigned, the fused tail path; ed_vector with every seventh entry zero: signed, vanishing
# amplitudes; conv_2d, 8 filters 3 x 3: pair correlations through the family's own row path
FAMILIES = ('fully_connected', 'ed_vector', 'conv_2d')


def _lists():
  """(pairs [120][2], masks [70][16], bonds (34), bond pairs [70][2])."""
  from cgs_vmc_amd import lattice
  from tests import test_gpu_dimer as td
  from tests import test_gpu_renyi as tr
  rng = np.random.default_rng(6)
  extra = np.random.default_rng(8).integers(0, 2, (70 - len(tr.MASKS), tr.N)).astype(np.uint8)
  masks = np.concatenate([tr.MASKS.astype(np.uint8), extra])          # more than one 64-thread fold block
  every = lattice.all_bond_pairs(len(td.BONDS34))
  bond_pairs = every[rng.permutation(len(every))[:70]]                # the 70 pairs of tests/test_gpu_dimer.py
  pairs = np.asarray(lattice.all_pairs(tr.N))
  assert pairs.shape == (120, 2) and masks.shape == (70, tr.N) and bond_pairs.shape == (70, 2)
  return pairs, masks, list(td.BONDS34), bond_pairs


def run_case(ansatz):
  """Runs the family on cuda:0 and returns {'<stage>/<quantity>': array}."""
  from tests import test_gpu_renyi as tr
  pairs, masks, bonds, bond_pairs = _lists()
  theta = tr._family(ansatz)[0]
  out = {}
  eng = tr._engine(ansatz)
  eng.set_params(theta); eng.set_configs(tr._cfg(2)); eng.set_bonds(tr.BONDS, 1.0, 1.0)

  def energies(tag):
    out[tag + '/eloc'] = eng.local_energy()[0]
    out[tag + '/diag'], out[tag + '/off'] = eng.local_energy_terms()

  def corr(tag, p, per=0):
    out['corr_%s/zz' % tag], out['corr_%s/ex' % tag] = eng.pair_correlations(p, pairs_per_pass=per)

  def renyi(tag, m, per=0):
    out['renyi_%s/swap' % tag], out['renyi_%s/match' % tag] = eng.renyi2_swap(m, regions_per_pass=per)

  def dimer(tag, b, p, per=0):
    out['dimer_%s/bond' % tag], out['dimer_%s/dd' % tag] = eng.dimer_correlations(b, p, pairs_per_pass=per)

  energies('eloc_before')
  # growth on one ctx: 3 items, the full list, 3 items again
  corr('first3', pairs[:3]); corr('full', pairs); corr('again3', pairs[5:8])
  renyi('first3', masks[:3]); renyi('full', masks); renyi('again3', masks[5:8])
  dimer('first3', bonds[:3], [(0, 1), (2, 0), (1, 1)]); dimer('full', bonds, bond_pairs)
  dimer('again3', bonds[5:8], [(2, 1), (0, 0), (1, 2)])
  # pass splits: 120 = 17 x 7 + 1, 70 = 64 + 6, 34 = 4 x 7 + 6 and 70 = 10 x 7
  corr('per7', pairs, 7)
  renyi('per64', masks, 64)
  dimer('per7', bonds, bond_pairs, 7)
  energies('eloc_after')
  eng.close()
  return out


def main():
  data = {}
  for name in FAMILIES:
    for k, v in run_case(name).items():
      data['{}/{}'.format(name, k)] = v
  np.savez_compressed(PATH, **data)
  print('wrote', PATH, os.path.getsize(PATH), 'bytes,', sum(v.size for v in data.values()), 'values')


if __name__ == '__main__':
  main()

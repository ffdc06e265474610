"""Records tests/golden/measure_bits_late.npz: what the four later measurements (vmc_symmetry_expectations,
vmc_projected_energy, vmc_energy_moments, vmc_overlap) return, bit for bit, on small fixed problems.
tests/test_gpu_measure_bits_late.py compares a build against it with assert_array_equal.

PROVENANCE: like measure_bits.npz these vectors are NOT oracle outputs.  They are the results of the library itself on
an MI355X, recorded at the commit before the seven entries of csrc/vmc_api_measure.hip were rewritten around one exit
guard and one row pass (a host-side change; no kernel, launch argument, buffer size or launch order touched).  Every
value is an fp64 sum folded in a fixed order, so they pin that order and the pass / buffer bookkeeping around it, not
the physics (which tests/test_gpu_symm.py, test_gpu_proj.py, test_gpu_moments.py and test_gpu_state_overlap.py check
against the oracles).  Re-record only when a change of the bits is intended:

  python tests/golden/make_measure_bits_late.py   # needs the GPU; rewrites tests/golden/measure_bits_late.npz

The generator runs every family twice and refuses to write when the two runs differ in any bit.

N = 16 on the 4 x 4 torus, B = 40 fixed chains (set_configs, no sampling), one ctx per family.  The ops are the 16
translations, the 7 non-identity elements of C4v, and the same 23 with the spin flip: 46 ops, each of which maps the 32
torus bonds onto themselves.  Per family the file holds `<family>/<stage>/<quantity>`, in the order of the calls:
  eloc_before, eloc_after / eloc, diag, off     local_energy() and local_energy_terms() under the torus Hamiltonian
  symm_<tag> / ratio                            symmetry_expectations
  proj_<tag> / w, we, e_sum, n_alive, rows      projected_energy and last_connected_rows() after it; the characters are
                                                default_rng(5).standard_normal((19, n_ops)): two sector tiles of 16
  mom_<tag> / sums, e_loc, h2_loc, n_rows2      energy_moments(per_chain=True); sums = e, e2, g, eg, g2, n_alive
  overlap_<tag> / sums, ratio                   overlap(per_chain=True) against omega = the family at seed 1;
                                                sums = s1, s2, alive, log_scale
with <tag> = first3 (3 ops on the fresh ctx, 2 sectors: the buffers are allocated), full (all 46 ops, 19 sectors,
library's pass size: they grow), again3 (ops 5 .. 7, 2 sectors: they are larger than needed) and per7 (all 46 at 7 ops
per pass: 46 = 6 x 7 + 4); auto, per777 and per4096 for the rows per pass of the moments; first and again for the two
overlap calls.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, 'measure_bits_late.npz')
# fully_connected H = 32: unsigned, the fused tail path; ed_vector with every seventh entry zero: signed, vanishing
# amplitudes; conv_2d, 8 filters 3 x 3: the family's own row path
FAMILIES = ('fully_connected', 'ed_vector', 'conv_2d')
N_SECTORS = 19


def _ops():
  """(perms [46][16] int32, flips [46] uint8)."""
  from cgs_vmc_amd import lattice
  perms = np.concatenate([lattice.translations(4, 4), lattice.point_group(4, 4)[1][1:]])
  assert perms.shape == (23, 16)
  return np.ascontiguousarray(np.concatenate([perms, perms])), np.repeat(np.array([0, 1], np.uint8), 23)


def run_case(ansatz):
  """Runs the family on cuda:0 and returns {'<stage>/<quantity>': array}."""
  from cgs_vmc_amd import _hip
  from tests import test_gpu_renyi as tr
  perms, flips = _ops()
  out = {}
  eng = tr._engine(ansatz)
  eng.set_params(tr._family(ansatz)[0]); eng.set_configs(tr._cfg(2)); eng.set_bonds(tr.BONDS, 1.0, 1.0)

  def energies(tag):
    out[tag + '/eloc'] = eng.local_energy()[0]
    out[tag + '/diag'], out[tag + '/off'] = eng.local_energy_terms()

  def symm(tag, k, per=0):
    out['symm_%s/ratio' % tag] = eng.symmetry_expectations(perms[k], flips[k], ops_per_pass=per)

  def proj(tag, k, n_sectors, per=0):
    n_ops = len(perms[k])
    chi = np.random.default_rng(5).standard_normal((N_SECTORS, n_ops))[:n_sectors]
    r = eng.projected_energy(perms[k], flips[k], chi, ops_per_pass=per)
    out['proj_%s/w' % tag], out['proj_%s/we' % tag] = r['w_sum'], r['we_sum']
    out['proj_%s/e_sum' % tag] = np.float64(r['e_sum'])
    out['proj_%s/n_alive' % tag] = np.int64(r['n_alive'])
    out['proj_%s/rows' % tag] = np.int64(eng.last_connected_rows())

  def moments(tag, per):
    r = eng.energy_moments(rows_per_pass=per, per_chain=True)
    out['mom_%s/sums' % tag] = np.array([r[q] for q in ('e_sum', 'e2_sum', 'g_sum', 'eg_sum', 'g2_sum', 'n_alive')], np.float64)
    out['mom_%s/e_loc' % tag], out['mom_%s/h2_loc' % tag] = r['e_loc'], r['h2_loc']
    out['mom_%s/n_rows2' % tag] = np.int64(r['n_rows2'])

  def overlap(tag):
    r = eng.overlap(per_chain=True)
    out['overlap_%s/sums' % tag] = np.array([r[q] for q in ('s1', 's2', 'alive', 'log_scale')], np.float64)
    out['overlap_%s/ratio' % tag] = r['ratio']

  energies('eloc_before')
  every = slice(None)
  # growth on one ctx: 3 ops, all 46, 3 ops again; then the pass split with a ragged last pass
  symm('first3', slice(0, 3)); symm('full', every); symm('again3', slice(5, 8)); symm('per7', every, 7)
  proj('first3', slice(0, 3), 2); proj('full', every, N_SECTORS); proj('again3', slice(5, 8), 2)
  proj('per7', every, N_SECTORS, 7)
  moments('auto', 0); moments('per777', 777); moments('per4096', 4096)
  eng.set_params(tr._family(ansatz, seed=1)[0], _hip.VMC_OMEGA)
  overlap('first'); overlap('again')
  eng.local_energy()
  energies('eloc_after')
  eng.close()
  return out


def main():
  data = {}
  for name in FAMILIES:
    first, second = run_case(name), run_case(name)
    assert sorted(first) == sorted(second)
    differ = [k for k in sorted(first) if np.asarray(first[k]).tobytes() != np.asarray(second[k]).tobytes()]
    if differ:
      raise SystemExit('{}: two runs differ in {}: nothing written'.format(name, differ))
    for k, v in first.items():
      data['{}/{}'.format(name, k)] = np.asarray(v)
  np.savez_compressed(PATH, **data)
  print('wrote', PATH, os.path.getsize(PATH), 'bytes,', sum(v.size for v in data.values()), 'values')


if __name__ == '__main__':
  main()

"""Records tests/golden/fourspin_bits.npz: what a ctx with four-spin (J-Q) terms returns, bit for bit, on small fixed
problems.  tests/test_gpu_fourspin_bits.py compares a build against it with assert_array_equal.

PROVENANCE: like measure_bits.npz these vectors are NOT oracle outputs.  They are the results of the library itself on
an MI355X, recorded at the commit before the kernels of csrc/fourspin.hip, moments.hip and dimer.hip were rewritten over
the shared device pieces of csrc/measure_dev.hpp (the row writer, the tile scan, the list walker).  The list is integer
work, the rows are copies of +-1 floats and the fold is an fp64 chain in a documented order, so the vectors pin the order
of the list, the prefix over the chains and the fold's chain of operations -- not the physics, which
tests/test_gpu_fourspin.py checks against the fp64 oracle.  Re-record only when a change of the bits is intended:

  python tests/golden/make_fourspin_bits.py   # needs the GPU; rewrites tests/golden/fourspin_bits.npz

The generator runs every case twice and refuses to write when the two runs differ in any bit.

The cases, each the smallest at which one of the shared pieces can go wrong:
  torus_<family>   the 4 x 4 torus, TERMS34 / Q34 of tests/test_gpu_fourspin.py (34 terms, 36 pairs), exchange sign -1,
                   B = 6 chains with the Neel chain first, for fully_connected (unsigned), ed_vector (vanishing
                   amplitudes: dead chains and rows with r = 0) and pbdg (signed).  The unsigned family also holds an
                   all-up chain -- no antiparallel pair, no row; the signed ones refuse a chain off Sz = 0, so theirs is
                   the two-domain chain with few rows.  Stages: rpp0 (the library's pass size) and inside (a pass size
                   that ends inside the first chain's rows).
  chain66          N = 66 sites, lattice.jq_chain_terms(66): pairs and terms past 64 lanes, the site axis of the row
                   writer past one wavefront; B = 5.  Stages: rpp0 and per65 (65 rows per pass).
  batch1030        fully_connected on the torus, B = 1030 chains: two tiles of the prefix scan (its carry), a batch that
                   is no multiple of 4 or 16.
Per stage the file holds `<case>/<stage>/<quantity>`:
  eloc      local_energy()[0]                                  fp32 [B]
  rows      last_four_spin_rows()                              int64 [2]
  diag, off local_energy_terms() -- the fold's PARTS variant   fp32 [B] each
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, 'fourspin_bits.npz')
FAMILIES = ('fully_connected', 'ed_vector', 'pbdg')
CASES = tuple('torus_' + f for f in FAMILIES) + ('chain66', 'batch1030')


def _neel16():
  return np.where((np.arange(16) % 4 + np.arange(16) // 4) % 2 == 0, 1.0, -1.0).astype(np.float32)


def _stage(eng, out, tag, terms, q, rpp):
  eng.set_four_spin_terms(terms, q, -1, rows_per_pass=rpp)
  out[tag + '/eloc'] = eng.local_energy()[0]
  out[tag + '/rows'] = np.array(eng.last_four_spin_rows(), np.int64)
  out[tag + '/diag'], out[tag + '/off'] = eng.local_energy_terms()


def _torus(ansatz, b, out, stages):
  from tests import fourspin_oracle as fo
  from tests import test_gpu_fourspin as tf
  from tests import test_gpu_renyi as tr
  cfg = tr._cfg(5, b)
  cfg[0] = _neel16()
  # all up where the family takes it, else two domains (Sz = 0: two rows of eight)
  cfg[1] = 1.0 if ansatz == 'fully_connected' else np.where(np.arange(16) < 8, 1.0, -1.0)
  eng = tr._engine(ansatz, b=b)
  eng.set_params(tr._family(ansatz)[0]); eng.set_configs(cfg); eng.set_bonds(tf.BONDS, -1.0, 1.0)
  pairs, tp = fo.pair_table(tf.TERMS34)
  anti = np.array([cfg[0, i] != cfg[0, j] for i, j in pairs])
  first = int(anti.sum() + (anti[tp[:, 0]] & anti[tp[:, 1]]).sum())       # the rows of the Neel chain
  assert first >= 64
  for tag in stages:
    _stage(eng, out, tag, tf.TERMS34, tf.Q34, {'rpp0': 0, 'inside': first - 7}[tag])
  eng.close()


def _chain66(out):
  from cgs_vmc_amd import lattice
  from cgs_vmc_amd.engine import VmcEngine
  from oracle import vmc_oracle as vo
  n, b, h = 66, 5, 32
  eng = VmcEngine(n, b, 2, h, seed=2024)
  eng.set_params(vo.init_params(n, h, 2, np.random.default_rng(0)))
  cfg = vo.random_configurations(n, b, np.random.RandomState(3))
  cfg[0] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)      # Neel: every term active
  cfg[1] = np.where(np.arange(n) < n // 2, 1.0, -1.0)      # one domain: no active term
  eng.set_configs(cfg); eng.set_bonds([tuple(x) for x in vo.chain_bonds(n)], -1.0, 1.0)
  q = np.random.default_rng(n).uniform(0.5, 1.5, n).astype(np.float32)
  _stage(eng, out, 'rpp0', lattice.jq_chain_terms(n), q, 0)
  _stage(eng, out, 'per65', lattice.jq_chain_terms(n), q, 65)
  eng.close()


def run_case(name):
  """Runs the case on cuda:0 and returns {'<stage>/<quantity>': array}."""
  out = {}
  if name == 'chain66':
    _chain66(out)
  elif name == 'batch1030':
    _torus('fully_connected', 1030, out, ('rpp0',))
  else:
    assert name.startswith('torus_') and name[6:] in FAMILIES, name
    _torus(name[6:], 6, out, ('rpp0', 'inside'))
  return out


def main():
  data = {}
  for name in CASES:
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

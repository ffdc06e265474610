"""Records tests/golden/tail_bits.npz: what the fused row kernel k_tail16 (csrc/tail16.hpp) returns, bit for
bit, on small fixed problems.  tests/test_gpu_tail_bits.py compares a build against it with assert_array_equal.

PROVENANCE: unlike the other fixtures of this directory these vectors are NOT oracle outputs.  They are the fp32
results of the library itself on an MI355X, recorded at the commit before the row kernel's gather went through
the bond-difference table; they pin the order of every fused multiply-add of the kernel, not the physics (which
tests/test_gpu_engine.py and its siblings check against the oracle).  Re-record only when a change of the bits
is intended:

  python tests/golden/make_tail_bits.py        # needs the GPU; rewrites tests/golden/tail_bits.npz

Per case the file holds `<case>/<stage>/eloc` (per-chain local energies), `<case>/<stage>/rows`
(last_connected_rows) and `<case>/<stage>/amp<k>` (logits of plain rows through vmc_amplitude).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import vmc_oracle as vo  # noqa: E402

PATH = os.path.join(HERE, 'tail_bits.npz')


def _j1j2_4x4():
  """4 x 4 torus: nearest neighbours (J1 = 1) and diagonals (J2 = 0.5), per-bond couplings."""
  nn = [tuple(b) for b in vo.torus_bonds(4, 4)]
  diag = []
  for y in range(4):
    for x in range(4):
      s = 4 * y + x
      diag.append((s, 4 * ((y + 1) % 4) + (x + 1) % 4))
      diag.append((s, 4 * ((y + 1) % 4) + (x - 1) % 4))
  bonds = nn + diag
  jx = np.array([1.0] * len(nn) + [0.5] * len(diag), np.float32)
  return bonds, -jx, jx


# name: ansatz, n_sites, H, num_layers, batch, bonds, hidden activation, row counts of the amplitude calls.
# H x H layers: num_layers - 1 (fully_connected) or num_layers (rbm).  Padded units: 64, 128, 256.
CASES = {
    'fc_h64_hh1': dict(n=16, h=64, L=2, b=40, bonds='torus4x4', amp=(7, 40)),             # the fused last block alone
    'fc_h100_hh2': dict(n=36, h=100, L=3, b=24, bonds='torus6x6', amp=(48, 144)),         # plain + last, padded to 128
    'fc_h256_hh3': dict(n=16, h=256, L=4, b=32, bonds='torus4x4', amp=(31, 144)),         # the ring crosses two plain layers
    'fc_h200_hh1': dict(n=12, h=200, L=2, b=16, bonds='chain', amp=(16, 48)),             # flagship instantiation, padded
    'fc_h128_hh1': dict(n=16, h=128, L=2, b=20, bonds='torus4x4', amp=(1, 33)),
    'fc_h64_hh3': dict(n=12, h=50, L=4, b=30, bonds='chain', amp=(17, 129)),
    'tanh_h128_hh2': dict(n=16, h=128, L=3, b=24, bonds='torus4x4', act='tanh', amp=(24, 130)),
    'rbm_h100_hh2': dict(n=16, h=100, L=2, b=40, bonds='torus4x4', ansatz='rbm', amp=(9, 200)),
    'rbm_h48_hh1': dict(n=12, h=48, L=1, b=36, bonds='chain', ansatz='rbm', amp=(36,)),
    # RATIO rows below 32: one chain of the 4 x 4 torus has at most 32 connected rows, every other wave exits at once
    'few_rows': dict(n=16, h=64, L=3, b=1, bonds='torus4x4', amp=(1,), rows_below=32),
    # RATIO rows that leave the last wave a single valid 16-row half (batch chosen from the configurations)
    'single_half': dict(n=16, h=128, L=2, b='single_half', bonds='torus4x4', amp=(16,)),
    # >= 3 tiles per workgroup (256 persistent workgroups): the descriptors of the tile after next run
    'many_tiles': dict(n=36, h=64, L=2, b=4096, bonds='torus6x6', amp=(300,), rows_above=3 * 256 * 128),
    'j1j2': dict(n=16, h=128, L=3, b=48, bonds='j1j2', amp=(48,)),
    # the supervisor's set after vmc_transfer_params, again after a parameter update and after a new bond list
    'omega': dict(n=16, h=128, L=3, b=40, bonds='torus4x4', amp=(40,), omega=True),
}


def _bonds(kind, n):
  if kind == 'chain':
    return vo.chain_bonds(n), -1.0, 1.0
  if kind == 'j1j2':
    return _j1j2_4x4()
  lx = int(kind[5])
  return vo.torus_bonds(lx, n // lx), -1.0, 1.0


def _connected(cfg, bonds):
  ij = np.asarray(bonds).reshape(-1, 2)
  return int((cfg[:, ij[:, 0]] != cfg[:, ij[:, 1]]).sum())


def run_case(name):
  """Runs the case on cuda:0 and returns {'<stage>/<quantity>': array}."""
  from cgs_vmc_amd import _hip
  from cgs_vmc_amd.engine import VmcEngine
  c = CASES[name]
  n, h, L = c['n'], c['h'], c['L']
  ansatz = c.get('ansatz', 'fully_connected')
  seed = 100 + sorted(CASES).index(name)
  rng = np.random.default_rng(seed)
  init = vo.rbm_init_params if ansatz == 'rbm' else vo.init_params
  theta = init(n, h, L, rng)
  theta = (theta + 0.05 * rng.standard_normal(theta.size)).astype(np.float32)
  bonds, jx, jz = _bonds(c['bonds'], n)
  b = c['b']
  if b == 'single_half':
    pool = vo.random_configurations(n, 64, np.random.RandomState(seed))
    b = next(k for k in range(2, 65) if 1 <= _connected(pool[:k], bonds) % 32 <= 16)
  cfg = vo.random_configurations(n, b, np.random.RandomState(seed))
  extra = vo.random_configurations(n, max(c['amp']), np.random.RandomState(seed + 1))
  out = {}
  eng = VmcEngine(n, b, L, h, nonlinearity=c.get('act', 'relu'), seed=2024, ansatz=ansatz)

  def stage(tag, which):
    eloc, _ = eng.local_energy(which)
    rows = eng.last_connected_rows()
    assert rows == _connected(cfg, eng_bonds[0])
    if 'rows_below' in c:
      assert rows < c['rows_below']
    if 'rows_above' in c:
      assert rows > c['rows_above']
    if c['b'] == 'single_half':
      assert 1 <= rows % 32 <= 16
    out[tag + '/eloc'] = eloc
    out[tag + '/rows'] = np.array([rows], np.int64)
    for k, m in enumerate(c['amp']):
      out['{}/amp{}'.format(tag, k)] = eng.amplitude(extra[:m], which)[0]

  eng_bonds = [bonds]
  eng.set_params(theta)
  eng.set_configs(cfg)
  eng.set_bonds(bonds, jx, jz)
  stage('psi', _hip.VMC_PSI)
  if c.get('omega'):
    eng.transfer_params()
    stage('omega', _hip.VMC_OMEGA)
    theta2 = (theta + 0.1 * rng.standard_normal(theta.size)).astype(np.float32)
    eng.set_params(theta2)                  # psi moves on, the supervisor keeps the old set
    stage('psi_updated', _hip.VMC_PSI)
    stage('omega_kept', _hip.VMC_OMEGA)
    eng.transfer_params()
    stage('omega_updated', _hip.VMC_OMEGA)
    eng_bonds[0] = vo.chain_bonds(n)        # a new bond list under unchanged parameters
    eng.set_bonds(eng_bonds[0], -0.7, 1.3)
    stage('psi_rebonded', _hip.VMC_PSI)
    stage('omega_rebonded', _hip.VMC_OMEGA)
  eng.close()
  return out


def main():
  data = {}
  for name in CASES:
    for k, v in run_case(name).items():
      data['{}/{}'.format(name, k)] = v
  np.savez_compressed(PATH, **data)
  print('wrote', PATH, os.path.getsize(PATH), 'bytes')


if __name__ == '__main__':
  main()

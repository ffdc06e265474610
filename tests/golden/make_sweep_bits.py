"""Records tests/golden/sweep_bits.npz: what the persistent sampler k_sweep16 (csrc/sweep16.hpp) leaves behind,
bit for bit, on small fixed problems.  tests/test_gpu_sweep_bits.py compares a build against it with
assert_array_equal.

PROVENANCE: like tail_bits.npz these vectors are NOT oracle outputs.  They are the results of the library itself
on an MI355X, recorded at the commit before the sampler's hand-over draw went to the one-instruction Philox
product and its step loop was peeled into cache pass / steady-state steps / final refresh; they pin the Philox
bits, the order of every floating-point operation of the kernel and the accept decisions, not the physics (which
tests/test_gpu_engine.py and its siblings check against the oracle).  Re-record only when a change of the bits
is intended:

  python tests/golden/make_sweep_bits.py        # needs the GPU; rewrites tests/golden/sweep_bits.npz

Every case goes through the public engine API only and launches the sampler three times:
  1. mc_steps on fresh chains          -> no cache: leading cache pass, steps, final refresh
  2. a log-overlap accumulate          -> the supervisor's cache by ONE n_steps = 0 launch (final refresh alone)
  3. mc_steps with the accepted count  -> cache loaded, steps, final refresh that hands the activations over
Per case the file holds `<case>/<quantity>`: the chains, both logit caches, the accepted count, the per-chain
local energies of both parameter sets (they read the z1 cache and, for psi, the sampler's bond census) and the
accumulators after each accumulate.  The accumulators are 2 P + 8 floats (megabytes at 256 units), so the file
keeps a fingerprint of them that moves with any single bit: see _fingerprint.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import vmc_oracle as vo  # noqa: E402

PATH = os.path.join(HERE, 'sweep_bits.npz')

# name: lattice lx x ly, H, num_layers, batch, [ansatz, hidden activation, output activation].
# H x H layers: num_layers - 1 (fully_connected) or num_layers (rbm).  Padded units: 64, 128, 256.
CASES = {
    'fc256_4x4_b16': dict(lx=4, ly=4, h=256, L=3, b=16),                   # baseline hand-over variant, W1 in LDS
    'fc256_4x4_b40': dict(lx=4, ly=4, h=256, L=3, b=40),                   # partial last tile
    'fc256_10x10': dict(lx=10, ly=10, h=256, L=3, b=48),                   # the flagship shape's variant
    'fc256_16x8': dict(lx=16, ly=8, h=256, L=3, b=32),                     # 32 site blocks: acceptance draw in its own call
    'fc256_12x12': dict(lx=12, ly=12, h=256, L=3, b=32),                   # five draws per lane, W1 out of LDS
    'fc200_4x4': dict(lx=4, ly=4, h=200, L=3, b=24),                       # padded to 256
    'fc256_L2': dict(lx=6, ly=6, h=256, L=2, b=24),                        # one H x H layer
    'fc256_L4': dict(lx=6, ly=6, h=256, L=4, b=24),                        # three H x H layers
    'fc64_4x4': dict(lx=4, ly=4, h=64, L=3, b=24),                         # four waves, no hand-over
    'fc128_6x6': dict(lx=6, ly=6, h=128, L=3, b=24),                       # four waves, no hand-over
    'rbm128_4x4': dict(lx=4, ly=4, h=128, L=1, b=24, ansatz='rbm'),        # log cosh epilogue, onsite term
    'tanh256_4x4': dict(lx=4, ly=4, h=256, L=3, b=24, act='tanh'),         # general (non-prefetching) variant
    'out_tanh256_4x4': dict(lx=4, ly=4, h=256, L=3, b=24, oact='tanh'),    # accept test in the linear domain
}
STEPS_COLD, STEPS_WARM = 3, 5


def _fingerprint(acc):
  """[sum, weighted sum] of the accumulators' 32-bit patterns modulo 2^64, 509 evenly spread entries as they are
  and the eight scalars at the end: a single flipped bit anywhere changes the first word (and the second says
  roughly where), the samples make a mismatch readable."""
  bits = np.ascontiguousarray(acc, np.float32).view(np.uint32).astype(np.uint64)
  with np.errstate(over='ignore'):
    sums = np.array([bits.sum(dtype=np.uint64), (bits * np.arange(1, bits.size + 1, dtype=np.uint64)).sum(dtype=np.uint64)])
  pick = np.linspace(0, acc.size - 9, 509).astype(np.int64)
  return sums, np.concatenate([acc[pick], acc[-8:]])


def run_case(name):
  """Runs the case on cuda:0 and returns {'<quantity>': array}."""
  from cgs_vmc_amd import _hip
  from cgs_vmc_amd.engine import VmcEngine
  c = CASES[name]
  n, h, L, b = c['lx'] * c['ly'], c['h'], c['L'], c['b']
  ansatz = c.get('ansatz', 'fully_connected')
  seed = 300 + sorted(CASES).index(name)
  rng = np.random.default_rng(seed)
  init = vo.rbm_init_params if ansatz == 'rbm' else vo.init_params
  theta_w = init(n, h, L, rng)
  theta_w = (theta_w + 0.05 * rng.standard_normal(theta_w.size)).astype(np.float32)
  theta = (theta_w + 0.02 * rng.standard_normal(theta_w.size)).astype(np.float32)
  bonds = vo.torus_bonds(c['lx'], c['ly'])
  cfg = vo.random_configurations(n, b, np.random.RandomState(seed))
  out = {}
  eng = VmcEngine(n, b, L, h, nonlinearity=c.get('act', 'relu'), output_activation=c.get('oact', 'exp'),
                  seed=2024, ansatz=ansatz)
  assert eng.sweep_tile(16) == 16               # small batches would otherwise go to k_sweep8
  eng.set_params(theta_w)
  eng.transfer_params()                         # the supervisor's set
  eng.set_params(theta)
  eng.set_configs(cfg)
  eng.set_bonds(bonds, -1.0, 1.0)
  eng.mc_steps(STEPS_COLD, want_accepted=False)                 # launch 1
  out['configs_cold'] = eng.get_configs()
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.1)          # launch 2 (n_steps = 0) is in here
  out['omega_logit'] = eng.amplitude(None, _hip.VMC_OMEGA)[0]
  out['omega_eloc'] = eng.local_energy(_hip.VMC_OMEGA)[0]
  out['acc_overlap_bits'], out['acc_overlap_sample'] = _fingerprint(eng.get_accumulators())
  accepted = eng.mc_steps(STEPS_WARM, want_accepted=True)       # launch 3
  assert 0 <= accepted <= STEPS_WARM * b
  out['accepted'] = np.array([accepted], np.int64)
  out['configs'] = eng.get_configs()
  assert (out['configs'].sum(1) == cfg.sum(1)).all()
  out['logit'] = eng.amplitude(None, _hip.VMC_PSI)[0]
  out['eloc'] = eng.local_energy(_hip.VMC_PSI)[0]
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)                 # reads the activations launch 3 handed over
  out['acc_energy_bits'], out['acc_energy_sample'] = _fingerprint(eng.get_accumulators())
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

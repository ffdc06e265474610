"""Records tests/golden/path_bits.json: what one fixed sequence of entry points returns, bit for bit, on every kernel path
of a ctx (vmc_debug_kernel_path 0 .. 10) and on every arm that differs inside a path.  tests/test_gpu_path_bits.py
compares a build against it with equality.

PROVENANCE: like measure_bits.npz these values are NOT oracle outputs.  They are the results of the library itself on an
MI355X, recorded at the commit before vmc_ctx's path flags (conv, conv_general, wide, wide_fast, split, split_sweep, pbdg,
nnb, edvec) became the one enum KernelPath and the family dispatch of csrc/vmc_api*.hip became switches over it.  That
change is host-side only: every ctx launches the kernels it launched before, in the same order, so nothing may move by a
bit, and the launch count of every timed region stays what it was.  Re-record only when a change of the bits is intended:

  python tests/golden/make_path_bits.py        # needs the GPU; rewrites tests/golden/path_bits.json

N = 16 on the 4 x 4 torus, B = 64 chains; the engines, parameters and seeds are those of tests/test_gpu_renyi.py,
test_gpu_buffers.py and test_gpu_prod.py.  A case runs the sequence of run_case with timing enabled from the start and
records `<step>/<quantity>`: scalars verbatim (floats as float.hex), arrays of at most 64 elements as their raw 32- or
64-bit words, larger arrays as the sha256 of their bytes and their first 8 words, and last the launch count of every
region name a Timer of csrc/ carries (REGIONS).

The generator runs every case twice and writes a quantity only if both runs agree bit for bit; a quantity that does not
reproduce at the recording commit itself is left out of that case and named in NOT_REPRODUCIBLE below.  Logits, local
energies, chains, accepted counts and launch counts (MUST_KEEP) have no free reduction order and are never left out.

NOT_REPRODUCIBLE at the recording commit: none.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, 'path_bits.json')
N, B = 16, 64
# every region name a Timer in csrc/ carries at the recording commit
REGIONS = ('z1', 'tail_amp', 'bond_list', 'tail_eloc', 'eloc_reduce', 'sweep', 'refresh', 'grad', 'adam', 'sr_matvec',
           'corr_fold', 'renyi_rows', 'renyi_forward', 'renyi_fold', 'dimer_rows', 'dimer_forward', 'dimer_fold',
           'symm_rows', 'symm_forward', 'symm_fold', 'proj_rows', 'proj_forward', 'proj_accum', 'proj_eloc', 'proj_fold')
# name -> (kernel path, environment of the create call)
CASES = {
    'fully_connected': (0, {}),
    'rbm': (0, {}),
    'fc300': (1, {}),
    'rbm300': (1, {}),
    'fc300_general': (2, {'CGS_VMC_WIDE_FAST': '0'}),
    'fc300_general_cos': (2, {'CGS_VMC_WIDE_FAST': '0'}),
    'conv_2d': (3, {}),
    'fc256_split_rows': (4, {'CGS_VMC_SPLIT_BF16': '1'}),
    'fc256_split_sweep': (5, {'CGS_VMC_SPLIT_BF16': '2'}),
    'conv72_general': (6, {'CGS_VMC_CONV_GENERAL_BLOCK_MB': '8'}),
    'conv8_general': (6, {'CGS_VMC_CONV_GENERAL': '1'}),
    'gnn': (6, {}),
    'pbdg': (7, {}),
    'fully_connected_nnb': (8, {}),
    'ed_vector': (9, {}),
    'prod_pbdg_fc': (10, {}),
}
# families with stochastic reconfiguration (the SR tuple of tests/test_gpu_buffers.py: the dense and the convolutional paths)
SR_PATHS = (0, 1, 2, 3, 4, 5, 6)
# quantities that may never be left out of a case (prefixes of the keys)
MUST_KEEP = ('path', 'amp/', 'eloc', 'sweep/', 'sweep2/', 'launches/')


def _make(name):
  """(engine, theta) of a case, created under the case's environment."""
  from cgs_vmc_amd.engine import VmcEngine
  from oracle import vmc_oracle as vo
  from tests import test_gpu_prod as tp
  from tests import test_gpu_renyi as tr
  rng = np.random.default_rng(3)
  if name in ('fc300', 'fc300_general', 'fc300_general_cos'):
    act = 'cos' if name.endswith('cos') else 'relu'
    return VmcEngine(N, B, 2, 300, nonlinearity=act, seed=2024), vo.init_params(N, 300, 2, rng)
  if name == 'rbm300':
    return VmcEngine(N, B, 1, 300, ansatz='rbm', seed=2024), vo.rbm_init_params(N, 300, 1, rng)
  if name.startswith('fc256'):
    return VmcEngine(N, B, 2, 256, seed=2024), vo.init_params(N, 256, 2, rng)
  if name == 'conv72_general':
    eng = VmcEngine(N, B, 2, 72, ansatz='conv_2d', kernel_size=3, size_x=4, size_y=4, seed=2024)
    return eng, vo.conv_init_params('conv_2d', (72, 3, 4, 4), 2, rng)
  if name == 'conv8_general':
    return tr._engine('conv_2d', b=B), tr._family('conv_2d')[0]
  if name == 'prod_pbdg_fc':
    specs, prod, _, _ = tp._pair('pbdg_fc')
    return tp._engine(specs, B), prod.theta.astype(np.float32)
  return tr._engine(name, b=B), tr._family(name)[0]


def _rec(x):
  """A JSON value that holds x bit for bit."""
  if isinstance(x, (bool, int, str, np.integer)):
    return int(x) if isinstance(x, np.integer) else x
  if isinstance(x, (float, np.floating)):
    return float(x).hex()
  a = np.ascontiguousarray(x)
  words = a.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
  if a.size <= 64:
    return {'dtype': str(a.dtype), 'shape': list(a.shape), 'words': [int(w) for w in words]}
  return {'dtype': str(a.dtype), 'shape': list(a.shape), 'sha256': hashlib.sha256(a.tobytes()).hexdigest(),
          'first8': [int(w) for w in words[:8]]}


def run_case(name):
  """Runs the case on cuda:0 and returns {'<step>/<quantity>': JSON value}."""
  from cgs_vmc_amd import _hip
  from cgs_vmc_amd import lattice
  from tests import test_gpu_buffers as tb
  from tests import test_gpu_renyi as tr
  path, env = CASES[name]
  saved = {k: os.environ.get(k) for k in env}
  os.environ.update(env)
  try:
    eng, theta = _make(name)
  finally:
    for k, v in saved.items():
      if v is None:
        del os.environ[k]
      else:
        os.environ[k] = v
  out = {}

  def put(key, value):
    out[key] = _rec(value)

  def sweep(tag):
    put(tag + '/accepted', eng.mc_steps(N))
    put(tag + '/configs', eng.get_configs())

  def energies(tag):
    eloc, mean = eng.local_energy()
    put(tag + '/eloc', eloc); put(tag + '/mean', mean)
    out[tag + '/diag'], out[tag + '/off'] = map(_rec, eng.local_energy_terms())

  try:
    eng.timing_enable(True)
    put('path', eng.kernel_path())
    assert eng.kernel_path() == path and eng.num_params == theta.size, (name, eng.kernel_path())
    cfg = tr._cfg(2, b=B)
    eng.set_params(theta); eng.set_configs(cfg); eng.set_bonds(tb.TORUS, 1.0, 1.0)
    out['amp/logit'], out['amp/psi'] = map(_rec, eng.amplitude())
    out['amp/logit7'], out['amp/psi7'] = map(_rec, eng.amplitude(cfg[:7]))
    energies('eloc')
    sweep('sweep')
    energies('eloc2')
    eng.reset_accumulators(); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    put('grad/acc', eng.get_accumulators())
    eng.transfer_params(); sweep('sweep2'); eng.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.1)
    put('itswo/acc', eng.get_accumulators())
    try:
      eng.update_norm()
    except (NotImplementedError, ValueError) as e:      # a family's refusal is part of the record
      put('norm/refused', str(e))
    put('norm/shift', eng.get_shift())
    put('adam/energy', eng.apply_adam(_hip.VMC_MODE_ENERGY_GRADIENT, 1e-2)); put('adam/params', eng.get_params())
    if path in SR_PATHS:
      eng.sr_reserve(2)
      eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT); eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
      put('sr/iterations', eng.sr_solve(1e-2, 1e-3, 8)[0]); put('sr/solution', eng.sr_get_solution())
      eng.sr_reserve(0)
    if path != 10:
      out['corr/zz'], out['corr/ex'] = map(_rec, eng.pair_correlations(tb.PAIRS[:5]))
      out['renyi/swap'], out['renyi/match'] = map(_rec, eng.renyi2_swap(tr.MASKS[:3]))
      out['dimer/bond'], out['dimer/dd'] = map(_rec, eng.dimer_correlations(tb.TORUS[:3], tb.BOND_PAIRS[:3]))
      put('symm/ratio', eng.symmetry_expectations(tb.PERMS))
      proj = eng.projected_energy(tb.PERMS, None, lattice.sector_characters(4, 4, False)[1])
      for k in sorted(proj):
        put('proj/' + k, proj[k])
    means, accepted = eng.evaluate(None, 2, 2, 2)
    put('eval/means', means); put('eval/accepted', accepted)
    for region in REGIONS:
      put('launches/' + region, eng.timing_get(region)[1])
  finally:
    eng.close()
  return out


def main():
  data = {}
  for name in CASES:
    first, second = run_case(name), run_case(name)
    assert sorted(first) == sorted(second)
    keep = {k: v for k, v in first.items() if second[k] == v}
    for k in sorted(set(first) - set(keep)):
      print('NOT REPRODUCIBLE: {}/{}'.format(name, k))
      assert not k.startswith(MUST_KEEP), (name, k)
    data[name] = keep
    print(name, len(keep), 'of', len(first), 'quantities', flush=True)
  with open(PATH, 'w') as f:
    json.dump(data, f, indent=0, sort_keys=True)
    f.write('\n')
  print('wrote', PATH, os.path.getsize(PATH), 'bytes')


if __name__ == '__main__':
  main()

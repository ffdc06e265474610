"""GPU: the device buffers of a ctx over whole life cycles (csrc/vmc_ctx.hpp: every one is a DevBuf the ctx owns).

One case per kernel family at the family's smallest test shape (16 sites, 64 chains).  A case runs six identical
create ... close cycles from fixed seeds, and every cycle walks through every lazily allocated buffer group its family
has: the bond list set twice with different bond counts (the bond-difference table of the row kernel regrows), external
amplitudes on 7 and then 40 rows (the row scratch regrows), sampler steps and a gradient accumulate (the gradient
path's buffers), the SR store reserved for 2, then 3 batches, one short solve and the store released (families with
SR), every measurement on two list sizes, vmc_evaluate on two sample counts.  Then:
  1. the energy mean and the accumulators of cycle 6 equal those of cycle 1 bit for bit: nothing of a ctx survives it
     and nothing a cycle reads is left unwritten;
  2. the device's free memory after cycle 6 is within 8 MB of its value after cycle 1 (cycle 1 absorbs the code
     objects and the runtime's pools; method and bound of tests/test_gpu_edvec.py's life-cycle test).
No case provokes an allocation failure."""
import numpy as np
import pytest

from cgs_vmc_amd import _hip
from cgs_vmc_amd import lattice
from oracle import vmc_oracle as vo
from tests import test_gpu_prod as tp
from tests import test_gpu_renyi as tr

pytestmark = pytest.mark.gpu
N, B = tr.N, 64
CHAIN = sorted(vo.chain_bonds(N))                   # 16 bonds, then the torus' 32: the tables regrow
TORUS = tr.BONDS
PAIRS = np.asarray(lattice.all_pairs(N))            # 120
PERMS = lattice.translations(4, 4)                  # 16
BOND_PAIRS = [(0, 1), (2, 0), (1, 1), (5, 9), (31, 4)]
CYCLES = 6
# families with stochastic reconfiguration (vmc_sr_reserve refuses the others) / with the measurements (a product has none)
SR = ('fully_connected', 'rbm', 'wide_general', 'conv_2d', 'conv_general', 'gnn')
CASES = ('fully_connected', 'rbm', 'wide_general', 'conv_2d', 'conv_general', 'gnn', 'pbdg', 'fully_connected_nnb',
         'ed_vector', 'prod_first', 'prod_factor_first')


def _make(case, monkeypatch):
  """(engine, theta) of a case; kernel_path() vouches for the family's path."""
  from cgs_vmc_amd.engine import VmcEngine
  rng = np.random.default_rng(3)
  if case == 'wide_general':                        # 300 units on the general wide path (not the fused 257 .. 512 one)
    monkeypatch.setenv('CGS_VMC_WIDE_FAST', '0')
    eng, theta, path = VmcEngine(N, B, 2, 300, seed=2024), vo.init_params(N, 300, 2, rng), 2
  elif case == 'conv_general':                      # 72 filters: beyond the fused kernels; small blocks, not 768 MB ones
    monkeypatch.setenv('CGS_VMC_CONV_GENERAL_BLOCK_MB', '8')
    eng = VmcEngine(N, B, 2, 72, ansatz='conv_2d', kernel_size=3, size_x=4, size_y=4, seed=2024)
    theta, path = vo.conv_init_params('conv_2d', (72, 3, 4, 4), 2, rng), 6
  elif case.startswith('prod'):
    specs, prod, _, _ = tp._pair('pbdg_fc')
    eng, theta, path = tp._engine(specs, B), prod.theta.astype(np.float32), 10
  else:
    eng, theta = tr._engine(case, b=B), tr._family(case)[0]
    path = {'fully_connected': 0, 'rbm': 0, 'conv_2d': 3, 'gnn': 6, 'pbdg': 7, 'fully_connected_nnb': 8, 'ed_vector': 9}[case]
  assert eng.kernel_path() == path and eng.num_params == theta.size
  return eng, theta


def _cycle(case, monkeypatch):
  """One life cycle -> (energy mean, accumulators as bits)."""
  eng, theta = _make(case, monkeypatch)
  cfg = tr._cfg(2, b=B)
  eng.set_params(theta); eng.set_configs(cfg)
  eng.set_bonds(CHAIN, 1.0, 1.0)
  eng.local_energy()
  eng.set_bonds(TORUS, 1.0, 1.0)
  eng.amplitude(cfg[:7]); eng.amplitude(cfg[:40])
  eng.mc_steps(N)
  mean = eng.local_energy()[1]
  eng.reset_accumulators()
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  if case in SR:
    eng.sr_reserve(2); eng.sr_reserve(3)
    eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
    eng.sr_solve(1e-2, 1e-3, 8)
    eng.sr_reserve(0)
  if not case.startswith('prod'):
    for n in (3, len(PAIRS)):
      eng.pair_correlations(PAIRS[:n])
    for n in (3, len(tr.MASKS)):
      eng.renyi2_swap(tr.MASKS[:n])
    eng.dimer_correlations(TORUS[:3], BOND_PAIRS[:3]); eng.dimer_correlations(TORUS, BOND_PAIRS)
    for n in (1, len(PERMS)):
      eng.symmetry_expectations(PERMS[:n])
  eng.evaluate(None, 2, 2, 2); eng.evaluate(None, 2, 5, 2)
  eng.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
  acc = eng.get_accumulators().view(np.uint32).copy()
  if case == 'prod_factor_first':                   # a factor destroyed before its product; close() takes the rest
    eng.children[0].close()
  eng.close()
  return mean, acc


@pytest.mark.parametrize('case', CASES)
def test_life_cycles_leave_nothing_behind(case, monkeypatch):
  import torch
  first = last = free1 = None
  for k in range(CYCLES):
    last = _cycle(case, monkeypatch)
    if k == 0:
      first = last
      torch.cuda.synchronize()
      free1 = torch.cuda.mem_get_info()[0]
  torch.cuda.synchronize()
  lost = free1 - torch.cuda.mem_get_info()[0]
  print('%s: energy mean %.9g, device memory lost over cycles 2 .. %d: %d bytes' % (case, first[0], CYCLES, lost))
  assert np.float64(last[0]).tobytes() == np.float64(first[0]).tobytes(), (first[0], last[0])
  np.testing.assert_array_equal(last[1], first[1])
  assert lost < (8 << 20)

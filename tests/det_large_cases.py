"""The inputs of the determinant tests above 64 pairs (n = N/2 > 64: a second column group in every loop of
csrc/pb_det.hpp, two chains or one per workgroup, the LDS opt-in at N = 256) and the bands measured on them by the
float32 emulations of tests/pbdg_oracle.py.  One place, so that tests/test_pbdg.py proves the conditions of the GPU
tests on the oracle alone, tests/test_gpu_det_large.py runs the same inputs on the kernels, and
tests/golden/make_det_large_bands.py recomputes the stored figures."""
import functools

import numpy as np

from oracle import vmc_oracle as vo
from tests import nnb_oracle as no
from tests import pbdg_oracle as po

SEED = 2024                                    # the engines' sampler seed

# N: chains, steps T of the longest launch.  Chains per workgroup: 2, 2, 1 -- five chains leave a wave idle at 2.
# T: every chain of the emulation accepts more than R + 10 moves at N = 160 (R = 80) and N = 256 (R = 128).
SAMPLER = {130: dict(b=5, steps=120), 160: dict(b=5, steps=480), 256: dict(b=4, steps=576)}

# python tests/golden/make_det_large_bands.py   (CPU, a quarter of a minute) prints the three tables below.
# max |rho_fp32 - rho_fp64| over every decision of sampler_emulation on sampler_inputs(N); delta = 4 x this
EMULATED_RATIO_ERROR = {130: 0.000293, 160: 0.00109, 256: 0.00363}
# max over rows of |E_fp32 - E_fp64| / (eps32 sum_q |term_q|) of local_energy_fp32 on eloc_inputs(N); c = 8 x this
EMULATED_ELOC_RATIO = {160: 32.1, 256: 106.0}
# max over rows of |E_fp32 - E_fp64| / (eps32 sum_q |term_q|) of no.exchange_terms in float32 on nnb_inputs(N); c = 8 x
EMULATED_NNB_ELOC_RATIO = {130: 22.7, 160: 16.7}
DELTA_FACTOR, ELOC_FACTOR = 4.0, 8.0

ELOC = {160: dict(lx=16, ly=10, b=5), 256: dict(lx=16, ly=16, b=4)}


def theta(n_sites, seed=8):
  lim = np.sqrt(3.0 / n_sites)
  return np.random.default_rng(seed).uniform(-lim, lim, n_sites * n_sites).astype(np.float32)


def sampler_inputs(n_sites):
  """(theta, initial chains, T)."""
  c = SAMPLER[n_sites]
  return theta(n_sites), vo.random_configurations(n_sites, c['b'], np.random.RandomState(9)), c['steps']


@functools.lru_cache(maxsize=None)
def emulation(n_sites):
  th, cfg, steps = sampler_inputs(n_sites)
  return po.sampler_emulation(th, cfg, SEED, steps)


def delta(n_sites):
  return DELTA_FACTOR * EMULATED_RATIO_ERROR[n_sites]


def eloc_inputs(n_sites):
  """(theta, chains, bonds, jx[nb], jz[nb]): nearest and next-nearest bonds of the torus (the wrap bonds give both
  parities of |a - b|, up to N - 16), per-bond couplings with jx = 0 on one bond and jx < 0 on another; jz in
  quarters, so that the float32 diagonal 0.25 jz s_i s_j sums without rounding."""
  c = ELOC[n_sites]
  bonds = vo.torus_bonds(c['lx'], c['ly'], next_nearest=True)
  rng = np.random.default_rng(10)
  jx = rng.uniform(0.5, 1.5, len(bonds)).astype(np.float32)
  jx[3], jx[len(bonds) - 2] = 0.0, -0.75
  jz = rng.choice(np.array([-0.5, 0.25, 0.75, 1.0, 1.25], np.float32), len(bonds))
  cfg = vo.random_configurations(n_sites, c['b'], np.random.RandomState(11))
  return theta(n_sites), cfg, bonds, jx, jz


def eloc_bound(n_sites, terms, diag):
  """c eps32 sum_q |term_q| per row, plus one rounding of the final sum (the diagonal itself is exact: jz in
  quarters)."""
  eps = np.finfo(np.float32).eps
  s = np.abs(terms).sum(1)
  return ELOC_FACTOR * EMULATED_ELOC_RATIO[n_sites] * eps * s + eps * (np.abs(diag) + s)


NNB_LAYERS, NNB_UNITS = 2, 16
NNB_TORUS = {130: (13, 10), 160: (16, 10)}


def nnb_inputs(n_sites):
  """(theta, five rows, bonds, jx[nb], jz[nb]) of the L = 2, H = 16 network: the default initialisation with the
  pairing layer's weights at a twentieth and the uniform pairing matrix as its bias -- a backflow correction of a few
  per cent, so that the amplitude ratios of neighbouring configurations are of order one and every term counts."""
  l, h = NNB_LAYERS, NNB_UNITS
  th = no.default_theta(n_sites, l, h, 1)
  ow, ob = no.offsets(n_sites, l, h)
  th[ow:ob] *= np.float32(0.05)
  th[ob:] = theta(n_sites, 12)
  bonds = vo.torus_bonds(*NNB_TORUS[n_sites])
  rng = np.random.default_rng(41)
  jx = rng.uniform(0.5, 1.5, len(bonds)).astype(np.float32)
  jx[5], jx[7] = 0.0, -1.0
  jz = rng.choice(np.array([-0.5, 0.5, 1.0], np.float32), len(bonds))
  return th, vo.random_configurations(n_sites, 5, np.random.RandomState(2)), bonds, jx, jz


def nnb_eloc_bound(n_sites, terms, diag):
  eps = np.finfo(np.float32).eps
  s = np.abs(terms).sum(1)
  return ELOC_FACTOR * EMULATED_NNB_ELOC_RATIO[n_sites] * eps * s + eps * (np.abs(diag) + s)

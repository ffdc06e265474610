"""Recomputes the figures stored in tests/det_large_cases.py: per sampler shape the largest |rho_fp32 - rho_fp64| of
tests/pbdg_oracle.sampler_emulation over the test's own decisions (with the acceptance rate, the accepted moves of the
laziest chain and the share of decisions inside delta), per local-energy shape the largest
|E_fp32 - E_fp64| / (eps32 sum |terms|) of the fresh-inverse float32 emulation, and the same figure of the nnb rows'
float32 emulation (tests/nnb_oracle.exchange_terms).  CPU only:

  python tests/golden/make_det_large_bands.py

Paste the printed tables into tests/det_large_cases.py; tests/test_pbdg.py then checks that they still match."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import det_large_cases as dc  # noqa: E402
from tests import nnb_oracle as no  # noqa: E402
from tests import pbdg_oracle as po  # noqa: E402


def ratio_error(n_sites):
  em = dc.emulation(n_sites)
  return float(np.abs(em['rho32'].astype(np.float64) - em['rho64']).max())


def eloc_ratio(n_sites):
  theta, cfg, bonds, jx, jz = dc.eloc_inputs(n_sites)
  ref = po.exchange_terms(theta, cfg, bonds, jx)
  e64 = po.diagonal_energy(cfg, bonds, jz) + ref.sum(1)
  e32 = po.local_energy_fp32(theta, cfg, bonds, jx, jz).astype(np.float64)
  return float((np.abs(e32 - e64) / (np.finfo(np.float32).eps * np.abs(ref).sum(1))).max())


def nnb_eloc_ratio(n_sites):
  theta, cfg, bonds, jx, jz = dc.nnb_inputs(n_sites)
  ref = no.exchange_terms(theta, cfg, bonds, jx, dc.NNB_LAYERS, dc.NNB_UNITS)
  t32 = no.exchange_terms(theta, cfg, bonds, jx, dc.NNB_LAYERS, dc.NNB_UNITS, np.float32)
  e32 = po.diagonal_energy(cfg, bonds, jz, np.float32) + t32.sum(1, dtype=np.float32)
  e64 = po.diagonal_energy(cfg, bonds, jz) + ref.sum(1)
  return float((np.abs(e32 - e64) / (np.finfo(np.float32).eps * np.abs(ref).sum(1))).max())


def main():
  errs = {n: ratio_error(n) for n in dc.SAMPLER}
  for n, e in errs.items():
    em = dc.emulation(n)
    inside = np.abs(em['rho64'] - np.sqrt(em['u'].astype(np.float64))) <= dc.DELTA_FACTOR * e
    print('# N = %d: acceptance %.3f, fewest accepted moves of a chain %d (R = %d), %d of %d decisions inside delta = %.3g'
          % (n, em['accept'].mean(), em['accept'].sum(0).min(), po.refresh_interval(n), inside.sum(), inside.size,
             dc.DELTA_FACTOR * e))
  print('EMULATED_RATIO_ERROR = {%s}' % ', '.join('%d: %.3g' % kv for kv in errs.items()))
  print('EMULATED_ELOC_RATIO = {%s}' % ', '.join('%d: %.3g' % (n, eloc_ratio(n)) for n in dc.ELOC))
  print('EMULATED_NNB_ELOC_RATIO = {%s}' % ', '.join('%d: %.3g' % (n, nnb_eloc_ratio(n)) for n in dc.NNB_TORUS))


if __name__ == '__main__':
  main()

"""GPU: the sample-space stochastic reconfiguration (cgs_vmc_amd/csrc/srgram.hip: the Gram matrix of the stored samples on
fp32 MFMA, conjugate gradients on the centred n x n system) against the fp64 references of tests/sr_gram_cases.py and the
oracle's dense solve, and against the parameter-space solver it stands beside.

Tolerances (those of tests/test_gpu_sr.py for the same class of sums: fp32 MFMA + a CG on the fp32 matrix against fp64;
tests/test_gpu_sr_gram_shapes.py goes on from here: more than 300 samples, a bound per element, the iterates one by one):
  Gram matrix   |d| <= 2e-4 * max|T_ref|
  CG solution   |d| <= 2e-3 * ||x_ref||_inf    (cond(C T C + n lambda I) is 90 .. 200 at these shapes)
  both solvers  |d| <= 4e-3 * ||x||_inf        (the two added)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import vmc_oracle as vo
from tests import sr_gram_cases as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 1e-2

# ansatz, N, H, L, B, stored batches, reserved batches
SHAPES = [
    ('fully_connected', 8, 16, 2, 24, 1, 1),     # n less than one tile
    ('fully_connected', 10, 30, 2, 37, 2, 2),    # ragged n = 74; K = 10 and K = 30, neither a multiple of 4
    ('fully_connected', 12, 40, 1, 48, 2, 3),    # single layer; store partly filled: row stride != rows
    ('fully_connected', 16, 32, 2, 100, 3, 3),   # n = 300: several tiles, diagonal and off-diagonal, ragged last tile
    ('fully_connected', 8, 272, 2, 24, 2, 2),    # the 257 .. 512-unit path, Hp > H
    ('fully_connected', 8, 520, 1, 16, 2, 2),    # the general dense path
    ('rbm', 16, 32, 1, 64, 3, 3),                # the onsite term
    ('rbm', 8, 24, 0, 24, 2, 2),                 # rbm at its smallest num_fc_layers
]
AGREE = [SHAPES[k] for k in (0, 1, 2, 3, 6)]
_IDS = ['{}-{}x{}x{}-b{}-{}of{}'.format(*s) for s in SHAPES]


class Case:
  pass


_CASES = {}


def _case(shape):
  """The engine with its store filled, and the fp64 references, once per shape (the references are never written)."""
  if shape in _CASES:
    return _CASES[shape]
  from cgs_vmc_amd.engine import VmcEngine
  ansatz, n, h, L, b, stored, reserved = shape
  rbm = ansatz == 'rbm'
  rng = np.random.default_rng(0)
  theta = (vo.rbm_init_params if rbm else vo.init_params)(n, h, L, rng)
  theta += (0.05 * rng.standard_normal(theta.size)).astype(np.float32)
  eng = VmcEngine(n, b, L, h, seed=2024, ansatz=ansatz)
  eng.set_params(theta)
  eng.set_bonds(vo.chain_bonds(n), -1.0, 1.0)
  eng.sr_reserve(reserved)
  eng.reset_accumulators()
  cfgs, elocs = [], []
  for k in range(stored):
    cfg = vo.random_configurations(n, b, np.random.RandomState(10 + k))
    eng.set_configs(cfg)
    eng.accumulate(0)
    cfgs.append(cfg)
    elocs.append(eng.local_energy()[0])
  assert eng.sr_num_stored() == stored
  c = Case()
  c.eng, c.theta, c.shape = eng, theta, shape
  c.cfgs = np.concatenate(cfgs, 0)
  c.e = np.concatenate(elocs, 0).astype(np.float64)
  c.t_ref = sg.gram_ref(theta, c.cfgs, h, L, ansatz)
  c.o = sg.per_sample_grads(theta, c.cfgs, h, L, ansatz)
  c.x_ref = sg.solve_samples_ref(c.o, c.e, LAM)
  _, c.it64 = sg.cg_samples_ref(c.t_ref, c.e, LAM, 1e-6, 2000)
  for a in (c.cfgs, c.e, c.t_ref, c.o, c.x_ref, c.theta):
    a.setflags(write=False)
  _CASES[shape] = c
  return c


def _restore(c):
  """Parameters back after a test that stepped them (the store keeps what was recorded)."""
  c.eng.set_params(c.theta)


@pytest.mark.parametrize('shape', SHAPES, ids=_IDS)
def test_gram_matches_fp64_formula(shape):
  c = _case(shape)
  n = c.cfgs.shape[0]
  t = c.eng.sr_debug_gram()
  assert t.shape == (n, n) and t.dtype == np.float32
  err, scale = np.abs(t - c.t_ref).max(), np.abs(c.t_ref).max()
  print('gram', shape, 'err', err, 'scale', scale)
  assert err <= 2e-4 * scale
  assert np.array_equal(t, t.T)
  assert np.array_equal(t, c.eng.sr_debug_gram())


@pytest.mark.parametrize('shape', SHAPES, ids=_IDS)
def test_solution_matches_direct_solve(shape):
  c = _case(shape)
  iters, res = c.eng.sr_solve_samples(LAM, 1e-6, 2000)
  x = c.eng.sr_get_solution()
  err, scale = np.abs(x - c.x_ref).max(), np.abs(c.x_ref).max()
  print('solve', shape, 'iters', iters, 'it64', c.it64, 'res', res, 'err', err, 'scale', scale)
  assert res <= 1e-4, (iters, res)
  assert np.all(np.isfinite(x))
  assert err <= 2e-3 * scale, (iters, res)
  assert abs(iters - c.it64) <= 2           # (2 it64 + 10 while the CG vectors were fp32; measured: 0 or 1 off)
  if c.theta.size <= 20000:
    ref = vo.sr_solve(c.o, c.e, LAM)       # dense fp64 solve of the explicit (S + lam I)
    assert np.abs(x - ref).max() <= 2e-3 * np.abs(ref).max()
  iters2, res2 = c.eng.sr_solve_samples(LAM, 1e-6, 2000)
  assert iters2 == iters and res2 == res
  assert np.array_equal(x, c.eng.sr_get_solution())


@pytest.mark.parametrize('shape', AGREE, ids=['{}-{}x{}x{}-b{}-{}of{}'.format(*s) for s in AGREE])
def test_agrees_with_parameter_space_solver(shape):
  c = _case(shape)
  c.eng.sr_solve(LAM, 1e-6, 2000)
  x_par = c.eng.sr_get_solution()
  c.eng.sr_solve_samples(LAM, 1e-6, 2000)
  x = c.eng.sr_get_solution()
  err, scale = np.abs(x - x_par).max(), np.abs(x_par).max()
  print('agree', shape, 'err', err, 'scale', scale)
  assert err <= 4e-3 * scale
  try:
    e_mean = c.eng.sr_apply(0.05)          # theta -= lr x
    assert np.isfinite(e_mean)
    np.testing.assert_allclose(c.eng.get_params(), c.theta - np.float32(0.05) * x, rtol=0, atol=1e-6)
  finally:
    _restore(c)


@pytest.mark.parametrize('jx', [1.0, -1.0])
def test_constant_psi(jx):
  """psi constant (every parameter zero but b_out): the centred Gram matrix vanishes.  Whether eps does is decided on the
  CPU by the closed form for a constant psi: it does for j_x = j_z (a constant is a total-spin eigenstate), not otherwise."""
  from cgs_vmc_amd.engine import VmcEngine
  n, h, b = 8, 16, 32
  bonds = vo.chain_bonds(n)
  theta = np.zeros(vo.num_params(n, h, 1), np.float32)
  theta[-1] = 0.3
  cfg = vo.random_configurations(n, b, np.random.RandomState(3))
  varies = np.ptp(vo.constant_psi_local_energy(cfg, bonds, jx, 1.0)) > 0
  assert varies == (jx != 1.0)
  eng = VmcEngine(n, b, 1, h, seed=1)
  eng.set_params(theta)
  eng.set_bonds(bonds, jx, 1.0)
  eng.sr_reserve(1)
  eng.reset_accumulators()
  eng.set_configs(cfg)
  eng.accumulate(0)
  iters, res = eng.sr_solve_samples(LAM, 1e-6, 100)
  x = eng.sr_get_solution()
  assert np.isfinite(res) and np.all(np.isfinite(x))
  if not varies:
    assert iters == 0 and res == 0.0 and not x.any()
  assert np.isfinite(eng.sr_apply(0.05))
  eng.close()


def test_refusals_leave_the_ctx_usable():
  from cgs_vmc_amd import _hip
  from cgs_vmc_amd.engine import VmcEngine
  n, h, L, b = 8, 16, 1, 64
  eng = VmcEngine(n, b, L, h, seed=5)
  eng.set_params(vo.init_params(n, h, L, np.random.default_rng(0)))
  eng.set_bonds(vo.chain_bonds(n), -1.0, 1.0)
  eng.set_configs(vo.random_configurations(n, b, np.random.RandomState(1)))
  with pytest.raises(_hip.HipLibraryError, match='vmc_sr_reserve'):
    eng.sr_solve_samples(LAM, 1e-6, 10)                 # no store
  with pytest.raises(_hip.HipLibraryError, match='vmc_sr_reserve'):
    eng.sr_debug_gram()
  eng.sr_reserve(257)
  eng.reset_accumulators()
  with pytest.raises(_hip.HipLibraryError, match='no samples'):
    eng.sr_solve_samples(LAM, 1e-6, 10)                 # nothing recorded
  eng.accumulate(0)
  for bad in (0.0, -1.0, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='diag_shift'):
      eng.sr_solve_samples(bad, 1e-6, 10)
  with pytest.raises(ValueError):
    eng.sr_solve_samples(LAM, -1.0, 10)
  with pytest.raises(ValueError):
    eng.sr_solve_samples(LAM, 1e-6, -1)
  iters, res = eng.sr_solve_samples(LAM, 1e-6, 200)     # ... and a valid call still works
  assert iters > 0 and res <= 1e-4
  x = eng.sr_get_solution()
  # more than 16,384 stored samples: 257 batches of 64 chains
  for _ in range(256):
    eng.accumulate(0)
  assert eng.sr_num_stored() * b == 16448
  with pytest.raises(NotImplementedError, match='vmc_sr_solve'):
    eng.sr_solve_samples(LAM, 1e-6, 10)
  with pytest.raises(NotImplementedError, match='vmc_sr_solve'):
    eng.sr_debug_gram()
  iters, res = eng.sr_solve(LAM, 1e-3, 200)             # the solver the message points to takes them
  assert iters > 0 and np.all(np.isfinite(eng.sr_get_solution()))
  eng.reset_accumulators()
  eng.accumulate(0)
  eng.sr_solve_samples(LAM, 1e-6, 200)
  assert np.array_equal(eng.sr_get_solution(), x)       # the same batch as before: the same bits
  eng.close()


def test_convolutional_store_is_refused():
  from cgs_vmc_amd.engine import VmcEngine
  rng = np.random.default_rng(8)
  geom = (8, 3, 4, 4)
  theta = vo.conv_init_params('conv_2d', geom, 2, rng)
  eng = VmcEngine(16, 12, 2, 8, seed=2024, ansatz='conv_2d', kernel_size=3, size_x=4, size_y=4)
  eng.set_params(theta)
  eng.set_bonds(vo.torus_bonds(4, 4), -1.0, 1.0)
  eng.sr_reserve(1)
  eng.reset_accumulators()
  eng.set_configs(vo.random_configurations(16, 12, np.random.RandomState(50)))
  eng.accumulate(0)
  with pytest.raises(NotImplementedError, match='vmc_sr_solve'):
    eng.sr_solve_samples(LAM, 1e-6, 10)
  with pytest.raises(NotImplementedError, match='vmc_sr_solve'):
    eng.sr_debug_gram()
  iters, res = eng.sr_solve(LAM, 1e-3, 200)
  assert iters > 0 and np.isfinite(eng.sr_apply(0.05))
  eng.close()


def test_sample_space_training_lowers_energy():
  """A few epochs on the 4x4 torus (exact E0 = -11.2285) with the sample-space solve; statistical, loose (mirrors
  test_gpu_sr.py::test_sr_training_lowers_energy)."""
  from cgs_vmc_amd.engine import VmcEngine
  n, h, L, b = 16, 32, 2, 256
  rng = np.random.default_rng(3)
  eng = VmcEngine(n, b, L, h, seed=7)
  eng.set_params(vo.init_params(n, h, L, rng))
  eng.set_bonds(vo.torus_bonds(4, 4), -1.0, 1.0)
  eng.set_configs(vo.random_configurations(n, b, np.random.RandomState(2)))
  eng.sr_reserve(4)
  energies = []
  for epoch in range(15):
    eng.mc_steps(5 * n)
    eng.update_norm(1e10)
    eng.reset_accumulators()
    for _ in range(4):
      eng.accumulate(0)
      eng.mc_steps(n)
    eng.sr_solve_samples(1e-2, 1e-3, 100)
    energies.append(eng.sr_apply(0.05))
  print('energies', energies)
  assert np.all(np.isfinite(energies))
  assert energies[-1] < energies[0], energies
  eng.close()


@pytest.mark.parametrize('solver', ['samples', None])
def test_run_training_with_either_solver(tmp_path, solver):
  """--optimizer=StochasticReconfiguration in a process of its own: CGS_VMC_SR_SOLVER=samples takes the sample-space
  solve, no variable the parameter-space one."""
  from cgs_vmc_amd import lattice
  d = str(tmp_path)
  lattice.write_bonds(d, lattice.torus_bonds(4, 4))
  env = dict(os.environ, CGS_VMC_SEED='77', CGS_VMC_CONFIG_SEED='5', CGS_VMC_INIT_SEED='31',
             PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get('PYTHONPATH')] if p]))
  env.pop('CGS_VMC_SR_SOLVER', None)
  if solver:
    env['CGS_VMC_SR_SOLVER'] = solver
  hp = ('batch_size=128,fc_layer_size=32,num_fc_layers=2,num_equilibration_sweeps=2,num_batches_per_epoch=4,'
        'learning_rates=[0.05],learning_rate_stops=[],sr_diag_shift=0.01,sr_cg_tolerance=0.001,sr_cg_max_iterations=100')
  p = subprocess.run([sys.executable, '-m', 'cgs_vmc_amd.run_training', '--checkpoint_dir', d, '--num_sites', '16',
                      '--heisenberg_jx', '-1.0', '--wavefunction_type', 'fully_connected',
                      '--optimizer', 'StochasticReconfiguration', '--num_epochs', '3', '--hparams', hp],
                     cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
  assert p.returncode == 0, p.stdout.decode()[-3000:]
  energies = [float(x) for x in open(os.path.join(d, 'metrics.txt')).read().split()]
  assert len(energies) == 3 and np.all(np.isfinite(energies)), energies

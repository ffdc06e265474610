"""CPU: the Lanczos-step energies without a GPU -- the fp64 oracle tests/moments_oracle.py against dense matrices, the
rules of the compacted second-order list, the algebra of LanczosStepEvaluator on scripted sums, the file of
run_lanczos_evaluation, and the planner (plan.hpp: plan_moment_*) under AddressSanitizer + UndefinedBehaviourSanitizer
in a program of its own (csrc/hostcheck_moments.cpp)."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from cgs_vmc_amd import evaluation
from cgs_vmc_amd import lattice
from cgs_vmc_amd import parallel
from cgs_vmc_amd import session as session_lib
from oracle import vmc_oracle as vo
from tests import moments_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING8 = [tuple(b) for b in lattice.chain_bonds(8)]
TORUS24 = [tuple(b) for b in vo.torus_bonds(2, 4)]            # the raw list of the 2-wide torus: twin bonds
PENDANT = [(0, 1), (1, 2), (0, 2), (2, 3)]                    # a triangle and a pendant bond


def _vector_psi(basis_index, vec):
  return lambda cfg: np.array([vec[basis_index[tuple(float(s) for s in row)]] for row in np.asarray(cfg)])


def _list_form_g(psi, x, bonds, hx, qz):
  """g(x) written out over the compacted list of second_order_rows: the statement the kernels implement."""
  first, rows, selfs = mo.second_order_rows(x, bonds)
  own = psi(np.array([x]))[0]
  diag = lambda y: sum(qz[b] * y[i] * y[j] for b, (i, j) in enumerate(bonds))
  r = lambda y: psi(np.array([y], np.float32))[0] / own
  e = diag(x) + sum(hx[a] * r(xa) for a, xa in first)
  g = diag(x) * e + sum(hx[a] * r(xa) * diag(xa) for a, xa in first)
  g += sum(hx[a] * hx[b] for a, b in selfs)
  g += sum(mult * hx[a] * hx[b] * r(y) for a, b, mult, y in rows)
  return e, g


@pytest.mark.parametrize('name,n,bonds', [('ring', 8, RING8), ('torus 2x4', 8, TORUS24)])
def test_oracle_is_h_squared_on_a_random_signed_vector(name, n, bonds):
  rng = np.random.default_rng(5)
  jx = rng.uniform(0.5, 1.5, len(bonds)).astype(np.float32)
  jz = rng.uniform(-1.2, -0.4, len(bonds)).astype(np.float32)
  basis, h = mo.dense_h(n, bonds, jx, jz)
  assert len(basis) == 70 and np.array_equal(h, h.T)
  if name != 'ring':
    assert len(set(map(frozenset, bonds))) < len(bonds)                # twin bonds are in the list
  vec = rng.standard_normal(70)
  assert (vec < 0).any() and (vec > 0).any()
  psi = _vector_psi(mo.sz0_basis(n)[1], vec)
  e, g, alive = mo.local_values(psi, basis, bonds, jx, jz)
  assert alive.all()
  hv = h @ vec
  np.testing.assert_allclose(e, hv / vec, rtol=1e-12)
  np.testing.assert_allclose(g, (h @ hv) / vec, rtol=1e-12)
  # the compacted list says the same (a < b for disjoint bonds, twins without a row, one shared site: one row)
  hx, qz = mo.couplings(len(bonds), jx, jz)
  for k in (0, 17, 69):
    e_l, g_l = _list_form_g(psi, basis[k], bonds, hx, qz)
    assert abs(e_l - e[k]) <= 1e-12 * abs(e[k]) and abs(g_l - g[k]) <= 1e-12 * abs(g[k])
  if name != 'ring':
    assert any(a != b for x in basis for a, b in mo.second_order_rows(x, bonds)[2])   # rule 1 through a twin, not only a == b


TRIANGLE = [(0, 1), (1, 2), (0, 2)]                            # on four sites, site 3 idle: every two bonds share a site
STAR = [(0, 3), (1, 3), (2, 3)]                               # likewise


@pytest.mark.parametrize('name,bonds', [('triangle + pendant', PENDANT), ('triangle', TRIANGLE), ('star', STAR)])
def test_bonds_that_share_sites(name, bonds):
  """The identity on graphs whose bonds (nearly) all meet.  Two bonds of a graph pairwise share a site only on a triangle or
  a star, so the triangle with its pendant keeps ONE disjoint pair, (0, 1) and (2, 3): there every row counted twice must
  come from that pair; on the triangle and on the star alone the list holds no disjoint pair at all."""
  rng = np.random.default_rng(6)
  jx = rng.uniform(0.5, 1.5, len(bonds)).astype(np.float32)
  jz = rng.uniform(0.4, 1.2, len(bonds)).astype(np.float32)
  basis, h = mo.dense_h(4, bonds, jx, jz)
  vec = rng.standard_normal(len(basis))
  psi = _vector_psi(mo.sz0_basis(4)[1], vec)
  e, g, _ = mo.local_values(psi, basis, bonds, jx, jz)
  hv = h @ vec
  np.testing.assert_allclose(e, hv / vec, rtol=1e-12)
  np.testing.assert_allclose(g, (h @ hv) / vec, rtol=1e-12)
  hx, qz = mo.couplings(len(bonds), jx, jz)
  total = twice = 0
  for k, x in enumerate(basis):
    _, rows, selfs = mo.second_order_rows(x, bonds)
    assert all(a == b for a, b in selfs)
    for a, b, mult, _ in rows:
      assert mult == (2.0 if not set(bonds[a]) & set(bonds[b]) else 1.0)
      if mult == 2.0:
        assert name == 'triangle + pendant' and (bonds[a], bonds[b]) == ((0, 1), (2, 3))
        twice += 1
    total += len(rows)
    _, g_l = _list_form_g(psi, x, bonds, hx, qz)
    assert abs(g_l - g[k]) <= 1e-12 * max(abs(g[k]), 1.0)
  assert total == mo.n_rows2(basis, bonds) > 0
  assert (twice > 0) == (name == 'triangle + pendant')


# ---- the evaluator's algebra

def _sums(e, g):
  e, g = np.asarray(e, np.float64), np.asarray(g, np.float64)
  return np.array([e.sum(), (e * e).sum(), g.sum(), (e * g).sum(), (g * g).sum(), len(e)], np.float64)


def _two_level(theta):
  """A two-level system with energies -1 and 2 in its eigenbasis, psi = (cos theta, sin theta), sampled EXACTLY: chains in
  proportion to |psi|^2.  -> (sums of 1000 chains, h1 .. h4)."""
  levels = np.array([-1.0, 2.0])
  w = np.array([np.cos(theta) ** 2, np.sin(theta) ** 2])
  counts = np.rint(1000 * w).astype(int)
  e = np.repeat(levels, counts)                         # e(x) = E_x and g(x) = E_x^2 on an eigenbasis
  p = counts / counts.sum()
  return _sums(e, e * e), np.array([(p * levels ** n).sum() for n in (1, 2, 3, 4)])


def test_lanczos_step_on_a_two_level_toy_is_the_exact_ground_energy():
  sums, hn = _two_level(0.6)
  out = evaluation.lanczos_step(sums)
  np.testing.assert_allclose([out['h1'], out['h2'], out['h3'], out['h4']], hn, rtol=1e-14)
  assert abs(out['energy'] - hn[0]) < 1e-14 and abs(out['variance'] - (hn[1] - hn[0] ** 2)) < 1e-13
  assert out['h2_check'] == pytest.approx(out['h2'], rel=1e-14)
  # span{psi, H psi} is the whole space of two levels: one step lands on the ground state
  assert abs(out['lanczos_energy'] + 1.0) < 1e-12
  assert abs(out['lanczos_variance']) < 1e-10
  assert abs(out['extrapolated_energy'] + 1.0) < 1e-10
  # alpha: (1 + alpha H) psi has no weight on the level 2
  assert abs(1.0 + 2.0 * out['alpha']) < 1e-10
  # and the generalised eigenproblem solved by numpy says the same
  a = np.array([[hn[0], hn[1]], [hn[1], hn[2]]]); s = np.array([[1.0, hn[0]], [hn[0], hn[1]]])
  assert abs(out['lanczos_energy'] - np.linalg.eigvals(np.linalg.solve(s, a)).real.min()) < 1e-11


def test_lanczos_step_three_levels_against_dense_numpy():
  levels = np.array([-2.0, 0.5, 3.0]); p = np.array([0.7, 0.2, 0.1])
  h = np.diag(levels); v = np.sqrt(p)
  hn, e1, alpha, var1 = mo.exact_moments(h, v)
  out = evaluation.lanczos_step(np.array([hn[0], hn[1], hn[1], hn[2], hn[3], 1.0]))
  assert abs(out['lanczos_energy'] - e1) < 1e-12 and abs(out['alpha'] - alpha) < 1e-12
  assert abs(out['lanczos_variance'] - var1) < 1e-11
  assert -2.0 <= out['lanczos_energy'] < out['energy']                      # variational, and an improvement
  line = out['energy'] - out['variance'] * (e1 - out['energy']) / (var1 - out['variance'])
  assert abs(out['extrapolated_energy'] - line) < 1e-12


def test_degenerate_overlap_matrix_gives_no_nan():
  e = np.full(50, -3.25)
  for sums in (_sums(e, e * e), _sums(e * (1 + 1e-7 * np.linspace(-1, 1, 50)), e * e)):     # exact, and at fp32 resolution
    out = evaluation.lanczos_step(sums)
    assert all(np.isfinite(out[k]) for k in evaluation.LANCZOS_QUANTITIES), out
    assert out['lanczos_energy'] == out['energy'] and out['alpha'] == 0.0
    assert out['extrapolated_energy'] == out['energy']
    assert abs(out['variance']) < 1e-12
  none = evaluation.lanczos_step(np.zeros(6))                                  # no chain alive: nan, never an exception
  assert all(np.isnan(none[k]) for k in evaluation.LANCZOS_QUANTITIES)


class _ScriptedEngine:
  """Engine double: energy_moments returns the next scripted dict; run_many counts the sampler's calls."""

  def __init__(self, script):
    self.script, self.at, self.steps = list(script), 0, []

  def energy_moments(self, which=0, rows_per_pass=0, per_chain=False):
    assert which == 0 and rows_per_pass == 0 and not per_chain
    s = self.script[self.at]
    self.at += 1
    return {'e_sum': s[0], 'e2_sum': s[1], 'g_sum': s[2], 'eg_sum': s[3], 'g2_sum': s[4], 'n_alive': int(s[5]),
            'n_rows2': 1234}

  def run_many(self, n):
    self.steps.append(n)


def _ops(engine, ensure=None):
  mc = session_lib.Op(lambda: None, 'mc_step')
  mc.last_accepted = 3
  mc.run_many = engine.run_many
  value = evaluation.EnergyMomentsTensor(engine, 0, ensure)
  return evaluation.EvalOps(value=value, mc_step=mc, acceptance_rate=None, placeholder_input=None, wavefunction_value=None)


def _hparams(n_samples, batch=64):
  return types.SimpleNamespace(num_sites=8, batch_size=batch, num_equilibration_sweeps=5, num_monte_carlo_sweeps=2,
                               num_evaluation_samples=n_samples)


def _script(n_samples, seed, batch=64):
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(n_samples):
    e = -3.0 + 0.4 * rng.standard_normal(batch)
    out.append(_sums(e, e * e + 0.1 * rng.standard_normal(batch)))
  return out


def test_evaluator_jackknife_by_hand_and_single_sample():
  n = 6
  script = _script(n, 1)
  ensured = []
  eng = _ScriptedEngine(script)
  ev = evaluation.LanczosStepEvaluator()
  out = ev.run_evaluation(_ops(eng, lambda: ensured.append(1)), session_lib.Session(), _hparams(n), epoch_num=0)
  assert eng.at == n == len(ensured) and eng.steps == [5 * 8] + [2 * 8] * n and ev.acceptance_count == 3 * n
  assert set(out) == {k + s for k in evaluation.LANCZOS_QUANTITIES for s in ('', '_err')} | {'samples', 'n_rows2'}
  np.testing.assert_array_equal(out['samples'], np.array(script))
  assert out['n_rows2'] == 1234
  total = np.array(script).sum(0)
  whole = evaluation.lanczos_step(total)
  left = [evaluation.lanczos_step(total - s) for s in script]
  for k in evaluation.LANCZOS_QUANTITIES:
    assert out[k] == whole[k]
    th = np.array([l[k] for l in left])
    err = np.sqrt((n - 1) / n * ((th - th.mean()) ** 2).sum())
    assert out[k + '_err'] == pytest.approx(err, rel=1e-9, abs=1e-15), k
    assert out[k + '_err'] > 0
  one = evaluation.LanczosStepEvaluator().run_evaluation(_ops(_ScriptedEngine(script[:1])), session_lib.Session(),
                                                         _hparams(1), epoch_num=0)
  for k in evaluation.LANCZOS_QUANTITIES:
    assert one[k + '_err'] == 0.0 and np.isfinite(one[k])


def test_jackknife_errors_are_zero_for_identical_samples():
  script = [_script(1, 2)[0]] * 5
  out = evaluation.LanczosStepEvaluator().run_evaluation(_ops(_ScriptedEngine(script)), session_lib.Session(), _hparams(5),
                                                         epoch_num=0)
  for k in evaluation.LANCZOS_QUANTITIES:
    assert out[k + '_err'] == 0.0, (k, out[k + '_err'])
    assert np.isfinite(out[k])


def test_evaluator_two_ranks_of_scripted_shards_give_the_unsharded_result(monkeypatch):
  n = 4
  mine, theirs = _script(n, 3), _script(n, 4)
  reduced = []

  def fake_allreduce(values, op='sum'):
    values = np.asarray(values)
    assert op == 'sum' and values.dtype == np.float64 and values.shape == (6,)
    reduced.append(values.copy())
    return values + theirs[len(reduced) - 1]
  monkeypatch.setattr(parallel, 'world_size', lambda: 2)
  monkeypatch.setattr(parallel, 'allreduce_array', fake_allreduce)
  sharded = evaluation.LanczosStepEvaluator().run_evaluation(_ops(_ScriptedEngine(mine)), session_lib.Session(),
                                                             _hparams(n, 128), epoch_num=0)
  assert len(reduced) == n                              # one collective per sample, on the six fp64 sums
  monkeypatch.setattr(parallel, 'world_size', lambda: 1)
  whole = [a + b for a, b in zip(mine, theirs)]
  single = evaluation.LanczosStepEvaluator().run_evaluation(_ops(_ScriptedEngine(whole)), session_lib.Session(),
                                                            _hparams(n, 128), epoch_num=0)
  assert len(reduced) == n
  for k in evaluation.LANCZOS_QUANTITIES:
    assert sharded[k] == single[k] and sharded[k + '_err'] == single[k + '_err']


def test_driver_file_round_trips(tmp_path):
  from cgs_vmc_amd import run_lanczos_evaluation as rl
  out = evaluation.LanczosStepEvaluator().run_evaluation(_ops(_ScriptedEngine(_script(5, 7))), session_lib.Session(),
                                                         _hparams(5), epoch_num=0)
  path = rl.write_lanczos(str(tmp_path), out)
  assert os.path.basename(path) == 'lanczos.txt'
  back = rl.read_lanczos(path)
  assert list(back) == list(evaluation.LANCZOS_QUANTITIES)
  for k in evaluation.LANCZOS_QUANTITIES:
    assert back[k] == (out[k], out[k + '_err'])           # repr round-trips a double exactly
  with open(path) as f:
    lines = f.read().splitlines()
  assert lines[0].startswith('#') and len(lines) == 1 + len(evaluation.LANCZOS_QUANTITIES)
  assert all(len(l.split()) == 3 for l in lines[1:])
  flags = {row[0] for row in rl.FLAG_TABLE}
  assert {'checkpoint_dir', 'output_dir', 'hparams', 'j_x'} <= flags


def test_engine_and_library_declare_the_entry():
  from cgs_vmc_amd import _hip
  from cgs_vmc_amd.engine import VmcEngine
  assert 'vmc_energy_moments' in _hip.SIGNATURES and 'moments.hip' in _hip._SOURCES
  assert callable(VmcEngine.energy_moments)
  with open(os.path.join(ROOT, 'include', 'cgsvmc.h')) as f:
    assert 'int vmc_energy_moments(' in f.read()


@pytest.mark.skipif(shutil.which('g++') is None or shutil.which('make') is None, reason='needs g++ and make')
def test_moment_planner_under_asan_and_ubsan():
  p = subprocess.run(['make', '-C', os.path.join(ROOT, 'cgs_vmc_amd', 'csrc'), 'hostcheck_moments'],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
  out = p.stdout.decode()
  assert p.returncode == 0, out[-4000:]
  assert '-fsanitize=address,undefined' in out
  assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
  m = re.search(r'hostcheck_moments ok: (\d+) lists, (\d+) assertions', out)
  assert m, out[-2000:]
  assert int(m.group(1)) >= 64 and int(m.group(2)) > 10 ** 7

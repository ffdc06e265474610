"""The sampler's three entry points agree with one another on every kernel path: from one state, debug_proposals(step)
followed by mc_step_injected with exactly those proposals leaves the chains that mc_steps(1) leaves from a fresh engine in
the same state -- bit for bit --, the accept mask holds as many ones as mc_steps(1) counts, and local_energy() afterwards
is equal on both engines.  tests/test_gpu_path_bits.py pins mc_steps on every path but its recorded sequence never calls
the other two entries; the per-family oracle tests call them one family at a time.

The cases, engines, parameters, chains and bonds are those of tests/golden/make_path_bits.py (N = 16 on the 4 x 4 torus,
64 chains).  Every comparison is an equality; no fixture file.  The statement was checked against the library of the
commit before the samplers' host scaffold was shared (DESIGN_HISTORY.md H12) and held on all 16 cases there, so no case
is left out of the parametrisation."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_path_bits', os.path.join(_GOLDEN, 'make_path_bits.py'))
make_path_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_path_bits)


def _engine(name):
  """An engine of the case in the state make_path_bits.run_case starts from: parameters, chains, the torus bonds."""
  from tests import test_gpu_buffers as tb
  from tests import test_gpu_renyi as tr
  path, env = make_path_bits.CASES[name]
  saved = {k: os.environ.get(k) for k in env}
  os.environ.update(env)
  try:
    eng, theta = make_path_bits._make(name)
  finally:
    for k, v in saved.items():
      if v is None:
        del os.environ[k]
      else:
        os.environ[k] = v
  assert eng.kernel_path() == path
  eng.set_params(theta)
  eng.set_configs(tr._cfg(2, b=make_path_bits.B))
  eng.set_bonds(tb.TORUS, 1.0, 1.0)
  return eng


def _words(x):
  return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize('name', list(make_path_bits.CASES))
def test_injected_dump_is_one_plain_step(name):
  plain, inj = _engine(name), _engine(name)
  try:
    step = plain.step_counter
    assert step == inj.step_counter
    accepted = plain.mc_steps(1)
    i_up, i_dn, u = inj.debug_proposals(step)
    mask = inj.mc_step_injected(i_up, i_dn, u)
    assert np.array_equal(_words(inj.get_configs()), _words(plain.get_configs()))
    assert int(mask.sum()) == accepted
    (e_plain, m_plain), (e_inj, m_inj) = plain.local_energy(), inj.local_energy()
    assert np.array_equal(_words(e_inj), _words(e_plain))
    # (the words of the mean too: ed_vector's is nan over these chains, on both engines)
    assert np.array_equal(_words(np.float64(m_inj)), _words(np.float64(m_plain)))
  finally:
    inj.close()
    plain.close()

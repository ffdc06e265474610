"""The four later measurements keep their bits: symmetry expectations, projected energies, Lanczos moments and the
overlap of the cases of tests/golden/make_measure_bits_late.py against tests/golden/measure_bits_late.npz, which was
recorded on an MI355X before the entries of csrc/vmc_api_measure.hip were rewritten around one exit guard and one row
pass.  Every comparison is assert_array_equal: each value is an fp64 sum folded in a fixed order by kernels that rewrite
did not touch, so nothing may move by a single ulp.  The cases cover an unsigned family on the fused tail path, a signed
one with vanishing amplitudes and a convolutional one, device buffers that are first allocated, then grow, then are
larger than needed, ragged last passes, two sector tiles, three pass sizes of the second-order list, and the
Hamiltonian's local energies before and after all of it."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_measure_bits_late', os.path.join(_GOLDEN, 'make_measure_bits_late.py'))
make_measure_bits_late = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_measure_bits_late)


@pytest.fixture(scope='module')
def golden():
  with np.load(make_measure_bits_late.PATH) as f:
    return {k: f[k] for k in f.files}


@pytest.mark.parametrize('name', make_measure_bits_late.FAMILIES)
def test_measure_bits_late(name, golden):
  got = {k: np.asarray(v) for k, v in make_measure_bits_late.run_case(name).items()}
  want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + '/')}
  assert sorted(got) == sorted(want) and got
  for key in sorted(want):
    assert got[key].dtype == want[key].dtype, key
    np.testing.assert_array_equal(got[key], want[key], err_msg='{}/{}'.format(name, key))
  # a measurement moves nothing else: the Hamiltonian answers after all of them as before
  for q in ('eloc', 'diag', 'off'):
    np.testing.assert_array_equal(got['eloc_after/' + q], got['eloc_before/' + q])
  # pass splits do not move a bit either
  same = [('symm_full/' + q, 'symm_per7/' + q) for q in ('ratio',)]
  same += [('proj_full/' + q, 'proj_per7/' + q) for q in ('w', 'we', 'e_sum', 'n_alive', 'rows')]
  same += [('mom_auto/' + q, 'mom_' + tag + '/' + q) for tag in ('per777', 'per4096')
           for q in ('sums', 'e_loc', 'h2_loc', 'n_rows2')]
  # nor does a second call
  same += [('overlap_first/' + q, 'overlap_again/' + q) for q in ('sums', 'ratio')]
  for a, b in same:
    np.testing.assert_array_equal(got[a], got[b], err_msg='{} vs {}'.format(a, b))

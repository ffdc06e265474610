"""The three measurements keep their bits: pair correlations, Renyi-2 swap sums and dimer correlations of the cases of
tests/golden/make_measure_bits.py against tests/golden/measure_bits.npz, which was recorded on an MI355X before their C
entries were merged into csrc/vmc_api_measure.hip.  Every comparison is assert_array_equal: each value is an fp64 sum
folded over the chains in a fixed order by kernels the merge did not touch, so nothing may move by a single ulp.  The
cases cover an unsigned family on the fused tail path, a signed one with vanishing amplitudes and a convolutional one,
device buffers that are first allocated, then grow, then are larger than needed, ragged last passes in every pass
loop, and the Hamiltonian's local energies before and after all of it."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_measure_bits', os.path.join(_GOLDEN, 'make_measure_bits.py'))
make_measure_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_measure_bits)


@pytest.fixture(scope='module')
def golden():
  with np.load(make_measure_bits.PATH) as f:
    return {k: f[k] for k in f.files}


@pytest.mark.parametrize('name', make_measure_bits.FAMILIES)
def test_measure_bits(name, golden):
  got = make_measure_bits.run_case(name)
  want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + '/')}
  assert sorted(got) == sorted(want) and got
  for key in sorted(want):
    assert got[key].dtype == want[key].dtype, key
    np.testing.assert_array_equal(got[key], want[key], err_msg='{}/{}'.format(name, key))
  # a measurement moves nothing else: the Hamiltonian answers after all of them as before
  for q in ('eloc', 'diag', 'off'):
    np.testing.assert_array_equal(got['eloc_after/' + q], got['eloc_before/' + q])
  # pass splits do not move a bit either
  for a, b in (('corr_full/zz', 'corr_per7/zz'), ('corr_full/ex', 'corr_per7/ex'), ('renyi_full/swap', 'renyi_per64/swap'),
               ('renyi_full/match', 'renyi_per64/match'), ('dimer_full/bond', 'dimer_per7/bond'), ('dimer_full/dd', 'dimer_per7/dd')):
    np.testing.assert_array_equal(got[a], got[b])

"""The four-spin (J-Q) term pass keeps its bits: the cases of tests/golden/make_fourspin_bits.py against
tests/golden/fourspin_bits.npz, which was recorded on an MI355X before the kernels of csrc/fourspin.hip were rewritten
over the shared device pieces of csrc/measure_dev.hpp.  Every comparison is assert_array_equal on the integer views of the
values: the list is integer work, the rows are copies of +-1 floats and the fold is one fp64 chain in a documented
order, so nothing may move by a single ulp.  The cases cover an unsigned family, one with vanishing amplitudes and a
signed one on the 4 x 4 torus (with the Neel chain, a chain without rows, the library's pass size and one that ends
inside a chain), pairs, terms and sites past 64 lanes, and a batch past one tile of the prefix scan; each stage also goes
through vmc_local_energy_terms, the fold's second instantiation."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_fourspin_bits', os.path.join(_GOLDEN, 'make_fourspin_bits.py'))
make_fourspin_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_fourspin_bits)

_VIEW = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64, np.dtype(np.int64): np.uint64}


@pytest.fixture(scope='module')
def golden():
  with np.load(make_fourspin_bits.PATH) as f:
    return {k: f[k] for k in f.files}


@pytest.mark.parametrize('name', make_fourspin_bits.CASES)
def test_fourspin_bits(name, golden):
  got = {k: np.asarray(v) for k, v in make_fourspin_bits.run_case(name).items()}
  want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + '/')}
  assert sorted(got) == sorted(want) and got
  for key in sorted(want):
    assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
    view = _VIEW[want[key].dtype]
    np.testing.assert_array_equal(got[key].view(view), want[key].view(view), err_msg='{}/{}'.format(name, key))
  # the terms reach every live chain: the fixture is no record of a pass that did nothing
  assert got['rpp0/rows'].min() > 0
  # a pass size moves no bit
  for key in sorted(got):
    stage, q = key.split('/')
    if stage != 'rpp0':
      np.testing.assert_array_equal(got[key].view(_VIEW[got[key].dtype]), got['rpp0/' + q].view(_VIEW[got[key].dtype]),
                                    err_msg='{}: {} vs rpp0'.format(name, key))

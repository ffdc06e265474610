"""The fused row kernel k_tail16 keeps its bits: per-chain local energies, the connected-row count and plain
amplitude rows of the cases of tests/golden/make_tail_bits.py against tests/golden/tail_bits.npz, which was
recorded on an MI355X before the kernel's rank-2 gather was moved onto the bond-difference table.  Every
comparison is assert_array_equal: the table holds the very fp32 differences W1[i] - W1[j] the kernel used to
form per row, and no sum changed its order, so nothing may move by a single ulp.  The cases cover padded widths
64 / 128 / 256, one to three H x H layers, ratio and plain rows, rbm, tanh, fewer than 32 rows, a lone valid
half, more than three tiles per workgroup, per-bond couplings, and the supervisor's parameter set across
vmc_transfer_params, a parameter update and a new bond list (a stale table would show in each)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_tail_bits', os.path.join(_GOLDEN, 'make_tail_bits.py'))
make_tail_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_tail_bits)


@pytest.fixture(scope='module')
def golden():
  with np.load(make_tail_bits.PATH) as f:
    return {k: f[k] for k in f.files}


@pytest.mark.parametrize('name', sorted(make_tail_bits.CASES))
def test_tail_bits(name, golden):
  got = make_tail_bits.run_case(name)
  want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + '/')}
  assert sorted(got) == sorted(want) and got
  for key in sorted(want):
    assert got[key].dtype == want[key].dtype, key
    np.testing.assert_array_equal(got[key], want[key], err_msg='{}/{}'.format(name, key))

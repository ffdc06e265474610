"""The persistent sampler k_sweep16 keeps its bits: the chains, both logit caches, the accepted count, the
per-chain local energies (which read the sampler's z1 cache and bond census) and the accumulators after a
log-overlap and an energy-gradient accumulate (the latter from the activations the sampler hands over), for the
cases of tests/golden/make_sweep_bits.py against tests/golden/sweep_bits.npz, which was recorded on an MI355X
before the hand-over draw took the one-instruction Philox product and the step loop was peeled.  Every
comparison is assert_array_equal: both Philox forms give the same 32-bit words, and peeling moves no
floating-point operation, so nothing may move by a single ulp and no accept decision may flip.  Each case
launches the sampler without a cache (leading cache pass), as a pure refresh (n_steps = 0) and with a loaded
cache; the cases cover W1 in and out of LDS, a partial last tile, two and five draws per lane, the acceptance
draw in its own call, padded units, one to three H x H layers, the four-wave variants without hand-over, rbm,
a tanh hidden activation (general variant) and a non-exp output activation (general accept test)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_sweep_bits', os.path.join(_GOLDEN, 'make_sweep_bits.py'))
make_sweep_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_sweep_bits)


@pytest.fixture(scope='module')
def golden():
  with np.load(make_sweep_bits.PATH) as f:
    return {k: f[k] for k in f.files}


@pytest.mark.parametrize('name', sorted(make_sweep_bits.CASES))
def test_sweep_bits(name, golden):
  got = make_sweep_bits.run_case(name)
  want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + '/')}
  assert sorted(got) == sorted(want) and got
  for key in sorted(want):
    assert got[key].dtype == want[key].dtype, key
    np.testing.assert_array_equal(got[key], want[key], err_msg='{}/{}'.format(name, key))

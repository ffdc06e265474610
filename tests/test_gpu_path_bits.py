"""Every kernel path keeps its bits: the cases of tests/golden/make_path_bits.py -- one per value of kernel_path() and per
arm that differs inside a path -- against tests/golden/path_bits.json, which was recorded on an MI355X before the path
flags of vmc_ctx became the enum KernelPath and the family dispatch of csrc/vmc_api*.hip became switches over it.  Every
comparison is an equality: the change moved no kernel, launch argument, grid, stream or allocation size, so amplitudes,
local energies, chains, accepted counts, accumulators, parameters, SR solutions, the five measurements and the launch
count of every timed region are what they were."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_path_bits', os.path.join(_GOLDEN, 'make_path_bits.py'))
make_path_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_path_bits)


@pytest.fixture(scope='module')
def golden():
  with open(make_path_bits.PATH) as f:
    return json.load(f)


def test_the_fixture_holds_every_case_and_what_may_never_be_left_out(golden):
  assert sorted(golden) == sorted(make_path_bits.CASES)
  for name, want in golden.items():
    assert want['path'] == make_path_bits.CASES[name][0]
    for key in ('amp/logit', 'amp/logit7', 'eloc/eloc', 'eloc2/eloc', 'sweep/accepted', 'sweep/configs',
                'sweep2/accepted', 'sweep2/configs') + tuple('launches/' + r for r in make_path_bits.REGIONS):
      assert key in want, (name, key)


@pytest.mark.parametrize('name', list(make_path_bits.CASES))
def test_path_bits(name, golden):
  got = json.loads(json.dumps(make_path_bits.run_case(name)))
  want = golden[name]
  assert got['path'] == make_path_bits.CASES[name][0]
  assert set(want) <= set(got) and want
  for key in sorted(want):
    assert got[key] == want[key], '{}/{}'.format(name, key)

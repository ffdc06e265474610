"""CPU side of the ed_vector ansatz (FullVector, wavefunctions.py:1001-1080): the oracle's Lin tables, the class's
variables, from_hparams, its deep copy, every validation error, the generator tool and the planner cases of hostcheck."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from cgs_vmc_amd import _hip, session, utils, wavefunctions
from tests import edvec_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _fresh_graph():
  session.reset_default_graph(); wavefunctions.reset_name_scope()
  yield
  session.reset_default_graph(); wavefunctions.reset_name_scope()


@pytest.mark.parametrize('n', [4, 8, 16])
def test_lin_tables_round_trip_the_whole_sector(n):
  top, bot, length = eo.lin_tables(n)
  cfg = eo.sz0_configurations(n)
  assert length == len(cfg) and top.shape == bot.shape == (1 << (n // 2),)
  idx = eo.index(cfg, top, bot)
  assert sorted(idx.tolist()) == list(range(length))                 # a bijection onto [0, C(n, n/2))
  vec = np.arange(length, dtype=np.float64)
  np.testing.assert_array_equal(eo.amplitude(vec, cfg, top, bot), idx)
  t, b = eo.half_words(cfg)
  assert (t == ((cfg[:, n // 2:] > 0) * (1 << np.arange(n // 2))).sum(1)).all()
  assert (b == ((cfg[:, :n // 2] > 0) * (1 << np.arange(n // 2))).sum(1)).all()
  wavefunctions.check_lin_tables(n, top, bot, length)


@pytest.mark.parametrize('n', [4, 8, 16])
def test_tables_of_oracle_and_tool_match_a_brute_force_enumeration(n):
  """Independent of both constructions: the sector's words in ascending order (top in the high bits) take the entries
  0, 1, 2, ... -- Lin's enumeration in ascending (top, bot) order, counted one word at a time."""
  from tools import make_ed_vector as mk
  h = n // 2
  words = np.array([w for w in range(1 << n) if bin(w).count('1') == h])
  for top, bot, length in (eo.lin_tables(n), mk.lin_tables(n)):
    assert length == len(words)
    idx = np.asarray(top, np.int64)[words >> h] + np.asarray(bot, np.int64)[words & ((1 << h) - 1)]
    np.testing.assert_array_equal(idx, np.arange(len(words)))
  np.testing.assert_array_equal(mk.sector_words(n), words)


def test_from_hparams_reads_the_three_files(tmp_path):
  n = 8
  top, bot, length = eo.lin_tables(n)
  vec = np.random.default_rng(0).standard_normal(length).astype(np.float32)
  np.savetxt(tmp_path / 't.txt', top, fmt='%d'); np.savetxt(tmp_path / 'b.txt', bot, fmt='%d')
  np.savetxt(tmp_path / 'v.txt', vec, fmt='%.9g')
  hp = utils.create_hparams(checkpoint_dir=str(tmp_path), num_sites=n, wavefunction_type='ed_vector',
                            top_lin_table_file='t.txt', bot_lin_table_file='b.txt', ed_vector_file='v.txt')
  wf = wavefunctions.build_wavefunction(hp)
  assert isinstance(wf, wavefunctions.FullVector) and wavefunctions.WAVEFUNCTION_TYPES['ed_vector'] is wavefunctions.FullVector
  names, shapes = wf._shapes()
  assert names == ['full_vector/ed_vector'] and shapes == [(length,)]
  np.testing.assert_array_equal(wf._initial_vector, vec)
  np.testing.assert_array_equal(wf._top_lin_table, top)
  assert wf._top_lin_table.dtype == np.int32 and wf._initial_vector.dtype == np.float32
  assert wf.normalize_batch(None) is None and wf.update_norm(None) is None
  spec = wf._engine_spec()
  assert spec['ansatz'] == 'ed_vector' and spec['layer_size'] == length
  assert spec['lin_tables'] == top.tobytes() + bot.tobytes()
  assert _hip.ANSATZ_IDS['ed_vector'] == 10 and 'vmc_set_lin_tables' in _hip.SIGNATURES


def test_deepcopy_twin():
  n = 4
  top, bot, length = eo.lin_tables(n)
  wf = wavefunctions.FullVector(n, top, bot, np.arange(1, length + 1, dtype=np.float32))
  twin = copy.deepcopy(wf)
  assert isinstance(twin, wavefunctions.FullVector) and twin is not wf
  assert twin._shapes()[0] == ['dc_full_vector/ed_vector']
  np.testing.assert_array_equal(twin._initial_vector, wf._initial_vector)
  assert twin._initial_vector is not wf._initial_vector
  assert twin._engine_spec() == wf._engine_spec()


def test_validation_errors_name_the_offender():
  n = 8
  top, bot, length = eo.lin_tables(n)
  vec = np.ones(length, np.float32)
  FV = wavefunctions.FullVector
  with pytest.raises(ValueError, match='num_sites must be even'):
    FV(7, top, bot, vec)
  with pytest.raises(ValueError, match='top_lin_table must be a 1-D table'):
    FV(n, top[:-1], bot, vec)
  with pytest.raises(ValueError, match='bot_lin_table must be a 1-D table'):
    FV(n, top, bot.reshape(4, 4), vec)
  with pytest.raises(ValueError, match='bot_lin_table must hold integers'):
    FV(n, top, bot.astype(np.float64), vec)
  with pytest.raises(ValueError, match='vector must be 1-D'):
    FV(n, top, bot, vec.reshape(-1, 2))
  with pytest.raises(ValueError, match=r'index 69 outside \[0, 69\)'):
    FV(n, top, bot, vec[:-1])
  low = bot.copy(); low[0] = -1                        # top = 1111, bot = 0000: index top[15] - 1 -- still inside
  FV(n, top, low, vec)
  t2 = top.copy(); t2[0] = -1                          # top = 0000 pairs with bot = 1111 (entry 0): index -1
  with pytest.raises(ValueError, match='index -1 outside'):
    FV(n, t2, bot, vec)
  t30, b30 = np.zeros(1 << 15, np.int32), np.zeros(1 << 15, np.int32)
  with pytest.raises(NotImplementedError, match='num_sites > 28'):
    FV(30, t30, b30, vec)
  with pytest.raises(NotImplementedError):             # mps stays a stub
    wavefunctions.build_wavefunction(utils.create_hparams(wavefunction_type='mps'))


def test_make_ed_vector_tool_writes_a_loadable_directory(tmp_path):
  from tools import make_ed_vector as mk
  d = str(tmp_path / 'ring')
  e0 = mk.main([d, '--lattice', 'chain', '--size', '8'])
  hp = utils.load_hparams(os.path.join(d, 'hparams.pbtxt'))
  assert hp.wavefunction_type == 'ed_vector' and hp.num_sites == 8
  wf = wavefunctions.build_wavefunction(hp)
  from cgs_vmc_amd import lattice
  bonds = lattice.load_bonds(d, 8)
  assert len(bonds) == 8
  top, bot, length = eo.lin_tables(8)
  np.testing.assert_array_equal(wf._top_lin_table, top); np.testing.assert_array_equal(wf._bot_lin_table, bot)
  e = eo.local_energy(wf._initial_vector, eo.sz0_configurations(8), top, bot, bonds, 1.0, 1.0)
  assert np.abs(e - e0).max() < 1e-5                     # (the file holds the fp32-rounded vector)
  assert abs(eo.vector_from_ed(8, bonds, 1.0, 1.0)[0] - e0) < 1e-9
  assert session.latest_checkpoint(d) == os.path.join(d, 'model_prior_0_epochs')
  d2 = str(tmp_path / 'rand')
  assert mk.main([d2, '--lattice', 'triangular', '--size', '2', '4', '--random']) is None
  v = np.genfromtxt(os.path.join(d2, 'ed_vector.txt'), dtype=np.float32)
  assert v.shape == (70,) and (v > 0).all()


def test_hostcheck_covers_the_edvec_planners():
  src = open(os.path.join(ROOT, 'cgs_vmc_amd', 'csrc', 'hostcheck.cpp')).read()
  assert 'edvec_grid();' in src and 'plan_edvec_check_tables' in src and 'plan_edvec_sweep_threads' in src
  out = subprocess.run(['make', '-C', os.path.join(ROOT, 'cgs_vmc_amd', 'csrc'), 'hostcheck'], capture_output=True, text=True)
  assert out.returncode == 0 and 'hostcheck ok' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_cabi_declares_and_binds_the_new_symbol():
  header = open(os.path.join(ROOT, 'include', 'cgsvmc.h')).read()
  assert 'int vmc_set_lin_tables(vmc_ctx* ctx, int32_t n_half' in header and 'VMC_ANSATZ_ED_VECTOR = 10' in header
  rc = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', os.path.join(ROOT, 'tests', 'test_cabi_loads.py')],
                      capture_output=True, text=True, cwd=ROOT)
  assert rc.returncode == 0, rc.stdout[-2000:]

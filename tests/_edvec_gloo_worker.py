"""Worker of tests/test_gpu_edvec.py::test_edvec_two_gloo_ranks_match_one_ctx: two gloo ranks sharing ONE GPU, each with
half of the chains of an ed_vector ctx.

Part 1, engine level: the rank's chains, local energies and accumulators against an unsharded ctx and the fp64 oracle
(tests/edvec_oracle.py); then vmc_allreduce_accumulators over the ranks, the reduced buffer against the oracle over ALL
chains.  Bounds (u = 2^-24): one side within (c + 2) u sum |terms| per entry, c the chains of that side on the entry
(test_gpu_edvec.py's header); the reduced sum adds one rounding: (c + 3) u sum |terms| with c over both sides.

Part 2, product routing: training.run_optimization_epoch -> vmc_epoch_*_dist and evaluation.run_evaluation ->
vmc_evaluate for a FullVector, epoch by epoch against an unsharded engine stepped op by op (the pattern of
tests/_dist_gpu_worker.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from cgs_vmc_amd import _hip, evaluation, graph_builders, lattice, operators, parallel, session, training, utils, wavefunctions  # noqa: E402
from cgs_vmc_amd.engine import VmcEngine  # noqa: E402
from tests import edvec_oracle as eo  # noqa: E402

U = 2.0 ** -24


def _gather_rows(local_rows):
  t = torch.from_numpy(np.ascontiguousarray(local_rows, np.float32))
  parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
  dist.all_gather(parts, t)
  return np.concatenate([p.numpy() for p in parts])


def _random_sz0(n, rows, seed):
  rng = np.random.default_rng(seed)
  cfg = -np.ones((rows, n), np.float32)
  for r in cfg:
    r[rng.permutation(n)[:n // 2]] = 1.0
  return cfg


def _worst(res, vec, cfg, top, bot, w, extra):
  """Worst error / bound of g1 and g2 against the oracle over the chains `cfg`: ((c + 2 + extra) u sum |terms|)."""
  p = len(vec)
  g1, g2, a1, a2, cnt = eo.accumulate(vec, cfg, top, bot, w)
  worst = 0.0
  for got, ref, mag in ((res[:p], g1, a1), (res[p:2 * p], g2, a2)):
    err = np.abs(got.astype(np.float64) - ref)
    assert (err[cnt == 0] == 0).all()
    worst = max(worst, (err[cnt > 0] / ((cnt + 2 + extra) * U * mag)[cnt > 0]).max())
  return worst


def engine_level(rank, world, coll):
  n, b = 8, 256
  lb = b // world
  mine_rows = slice(rank * lb, (rank + 1) * lb)
  bonds = [tuple(x) for x in lattice.chain_bonds(n)]
  top, bot, length = eo.lin_tables(n)
  rng = np.random.default_rng(25)
  vec = rng.standard_normal(length).astype(np.float32)
  vec_w = (vec + 0.3 * rng.standard_normal(length)).astype(np.float32)
  cfg = _random_sz0(n, b, 26)
  one = VmcEngine(n, b, 1, length, ansatz='ed_vector', lin_tables=(top, bot), seed=2024)
  mine = VmcEngine(n, lb, 1, length, ansatz='ed_vector', lin_tables=(top, bot), seed=2024, chain_offset=rank * lb)
  for eng, rows in ((one, cfg), (mine, cfg[mine_rows])):
    eng.set_params(vec); eng.set_params(vec_w, _hip.VMC_OMEGA); eng.set_bonds(bonds, 1.0, 1.0)
    eng.set_configs(rows)
    eng.mc_steps(20)
  chains = one.get_configs()
  np.testing.assert_array_equal(mine.get_configs(), chains[mine_rows])               # bit for bit
  psi = vec[eo.index(chains, top, bot)]
  assert (psi != 0).all()
  for mode, beta, label in ((_hip.VMC_MODE_ENERGY_GRADIENT, 0.0, 'EnergyGradient'),
                            (_hip.VMC_MODE_LOG_OVERLAP_ITSWO, 0.05, 'LogOverlapITSWO')):
    which = _hip.VMC_OMEGA if beta else _hip.VMC_PSI
    eloc = one.local_energy(which)[0]
    np.testing.assert_array_equal(mine.local_energy(which)[0].view(np.uint32), eloc[mine_rows].view(np.uint32))
    w = eo.itswo_ratio_fp32(psi, vec_w[eo.index(chains, top, bot)], eloc, beta) if beta else eloc
    for eng in (one, mine):
      eng.reset_accumulators(); eng.accumulate(mode, beta)
    p = length
    w_one = _worst(one.get_accumulators(), vec, chains, top, bot, w, 0)
    w_side = _worst(mine.get_accumulators(), vec, chains[mine_rows], top, bot, w[mine_rows], 0)
    mine.allreduce_accumulators_dist(coll)                                             # vmc_allreduce_accumulators
    red = mine.get_accumulators()
    w_red = _worst(red, vec, chains, top, bot, w, 1)
    print('rank %d ed_vector %s: error / bound one ctx %.3f, this side %.3f, all-reduced %.3f'
          % (rank, label, w_one, w_side, w_red))
    assert w_one <= 1.0 and w_side <= 1.0 and w_red <= 1.0, (label, w_one, w_side, w_red)
    # scalar slots: each side sums its chains in double and rounds once (k_scalar_accum), the all-reduce rounds once
    # more -- 3 u sum |E| leaves one rounding to spare -- and the counts are exact
    e64 = eloc.astype(np.float64)
    assert abs(red[2 * p] - e64.sum()) <= 3 * U * np.abs(e64).sum(), (label, red[2 * p], e64.sum())
    assert red[2 * p + 1] == b, red[2 * p:]
    if beta:
      r64 = w.astype(np.float64)
      assert abs(red[2 * p + 2] - r64.sum()) <= 3 * U * np.abs(r64).sum() and red[2 * p + 3] == b, red[2 * p:]
    every = _gather_rows(red[None, :])
    np.testing.assert_array_equal(every[0].view(np.uint32), every[rank].view(np.uint32))   # the same sums on every rank
  one.close(); mine.close()


def product_routing(rank, world, coll):
  n, b = 8, 256
  lb = b // world
  top, bot, length = eo.lin_tables(n)
  vec = np.random.default_rng(41).uniform(0.5, 1.5, length).astype(np.float32)
  for name in ('LogOverlapITSWO', 'EnergyGradient'):
    session.reset_default_graph()
    wavefunctions.reset_name_scope()
    hp = utils.create_hparams(wavefunction_type='ed_vector', num_sites=n, batch_size=b, num_equilibration_sweeps=2,
                              num_monte_carlo_sweeps=1, num_batches_per_epoch=3,
                              learning_rates=[1e-2, 1e-3], learning_rate_stops=[1])
    nb = hp.num_batches_per_epoch
    wf = wavefunctions.FullVector(n, top, bot, vec)
    ham = operators.HeisenbergHamiltonian(lattice.chain_bonds(n), -1.0, 1.0)
    opt = training.GROUND_STATE_OPTIMIZERS[name]()
    shared = {}
    ops = opt.build_opt_ops(wavefunction=wf, hamiltonian=ham, hparams=hp, shared_resources=shared)
    sess = session.Session()
    sess.run([session.global_variables_initializer(), session.local_variables_initializer()])
    cfg_var = shared[graph_builders.ResourceName.CONFIGS]
    assert cfg_var.local_batch == lb and cfg_var.chain_offset == lb * rank
    assert cfg_var._engine.kernel_path() == 9
    ref = VmcEngine(n, b, 1, length, ansatz='ed_vector', lin_tables=(top, bot), seed=77)
    ref.set_params(wf._get_theta())
    ref.set_configs(_gather_rows(cfg_var.eval()))
    ref.set_bonds(ham._bonds_list, -1.0, 1.0)
    for epoch in range(2):
      lr = training.piecewise_constant(epoch, [1], [1e-2, 1e-3])
      ref.mc_steps(2 * n)
      well = np.ones(length, bool)
      if name == 'LogOverlapITSWO':
        ref.transfer_params()
        for _ in range(nb):
          ref.mc_steps(n)
          ref.reset_accumulators()
          ref.accumulate(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, hp.time_evolution_beta)
          g = ref.get_gradient(_hip.VMC_MODE_LOG_OVERLAP_ITSWO)
          well &= (np.abs(g) > 1e-3 * np.abs(g).max()) | (g == 0)
          ref.apply_adam(_hip.VMC_MODE_LOG_OVERLAP_ITSWO, lr, 0.9, hp.beta2, 1e-8)
        e_ref = ref.mean_energy()
      else:
        ref.reset_accumulators()
        for _ in range(nb):
          ref.accumulate(_hip.VMC_MODE_ENERGY_GRADIENT)
          ref.mc_steps(n)
        e_ref = ref.mean_energy()
        g = ref.get_gradient(_hip.VMC_MODE_ENERGY_GRADIENT)
        well &= (np.abs(g) > 1e-3 * np.abs(g).max()) | (g == 0)
        ref.apply_adam(_hip.VMC_MODE_ENERGY_GRADIENT, lr, 0.9, hp.beta2, 1e-8)
        ref.reset_accumulators()
      energy = opt.run_optimization_epoch(ops, sess, hp, epoch)
      assert abs(energy - e_ref) < 2e-5 * max(1.0, abs(e_ref)), (name, epoch, energy, e_ref)
      np.testing.assert_array_equal(cfg_var.eval(), ref.get_configs()[lb * rank:lb * (rank + 1)])
      got, want = wf._get_theta(), ref.get_params()
      # (entries whose gradient nearly cancels take Adam's first steps in either direction: the pattern of
      # tests/_dist_gpu_worker.py; entries no chain visited have gradient 0 on both sides and do not move)
      assert np.abs(got - want)[well].max() < 5e-5 and well.sum() > 0.5 * well.size, \
          (name, epoch, np.abs(got - want)[well].max(), well.sum())
      ref.set_params(got)
      m, v, t = cfg_var._engine.get_adam_state()
      ref.set_adam_state(m, v, t)
    every = _gather_rows(wf._get_theta()[None, :])
    np.testing.assert_array_equal(every[0], every[rank])                                # identical step on every rank
    if name == 'EnergyGradient':
      hp.set_hparam('num_evaluation_samples', 5)
      ev = evaluation.MonteCarloOperatorEvaluator()
      eops = ev.build_eval_ops(wavefunction=wf, operator=ham, hparams=hp, shared_resources=shared)
      eng = cfg_var._engine
      start, step0 = cfg_var.eval().copy(), eng.step_counter
      fused = ev.run_evaluation(eops, sess, hp, 0)
      ref.set_params(wf._get_theta())
      ref.set_configs(_gather_rows(start)); ref.step_counter = step0
      m_ref, _ = ref.evaluate(None, 2 * n, 5, n)
      assert len(fused) == 5 and np.allclose(fused, m_ref, rtol=1e-6, atol=1e-6), (fused, m_ref)
    ref.close()


def main():
  os.environ.update(CGS_VMC_SEED='77', CGS_VMC_CONFIG_SEED='5')
  parallel.init_from_env('gloo')
  world, rank = parallel.world_size(), parallel.rank()
  assert world == int(os.environ['WORLD_SIZE']) == 2
  coll = parallel.collective()
  engine_level(rank, world, coll)
  product_routing(rank, world, coll)
  dist.barrier()
  dist.destroy_process_group()
  print('rank {} ok'.format(rank))


if __name__ == '__main__':
  main()

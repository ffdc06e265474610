"""Evaluation of optimized wavefunctions (mirror of cgs_vmc/evaluation.py, hot-path scope:
MonteCarloOperatorEvaluator)."""
from __future__ import annotations

import os
from typing import Any, Dict, List, NamedTuple

import numpy as np

from . import graph_builders
from . import operators
from . import parallel
from . import session as session_lib
from .training import _run_mc_steps

EvalOps = NamedTuple(
    'EvaluationOps', [
        ('value', session_lib.Op),
        ('mc_step', session_lib.Op),
        ('acceptance_rate', session_lib.Op),
        ('placeholder_input', session_lib.Op),
        ('wavefunction_value', session_lib.Op),
    ]
)
"""Named tuple of tensors representing evaluation components."""


class WavefunctionEvaluator():
  """Parents class for wavefunction evaluators (evaluation.py:27-71)."""

  def build_eval_ops(self, wavefunction, operator, hparams, shared_resources):
    raise NotImplementedError

  def run_evaluation(self, eval_ops, session, hparams, epoch_num: int) -> Any:
    raise NotImplementedError


def _fused_evaluation(eval_ops):
  """(engine, ensure_hamiltonian) when `eval_ops` are the handles build_eval_ops made -- the batch
  mean of a Hamiltonian's local value under the wavefunction that also drives mc_step on the same
  CONFIGS variable -- else None (the op-by-op loop serves anything else).  CGS_VMC_EVAL_FUSED=0
  forces the op-by-op loop."""
  if os.environ.get('CGS_VMC_EVAL_FUSED', '1') == '0':
    return None
  lv = getattr(eval_ops.value, 'local_value_tensor', None)
  mc = eval_ops.mc_step
  if not isinstance(lv, operators.LocalValueTensor) or not hasattr(mc, 'run_many'):
    return None
  if lv.configs is not getattr(mc, 'configs', None) or lv.wavefunction is not getattr(mc, 'wavefunction', None):
    return None
  if lv.wavefunction._which != 0 or not hasattr(lv.engine, 'evaluate'):
    return None
  return lv.engine, lambda: lv.configs._ensure_hamiltonian(lv.operator)


class MonteCarloOperatorEvaluator(WavefunctionEvaluator):
  """Operator evaluation by running MCMC (evaluation.py:74-152)."""

  def build_eval_ops(self, wavefunction, operator, hparams,
                     shared_resources: Dict[graph_builders.ResourceName, Any]) -> EvalOps:
    """evaluation.py:77-110."""
    batch_size = hparams.batch_size
    n_sites = hparams.num_sites

    configs = graph_builders.get_configs(shared_resources, batch_size, n_sites)
    mc_step, acc_rate = graph_builders.get_monte_carlo_sampling(
        shared_resources, configs, wavefunction)

    value = operators.reduce_mean(operator.local_value(wavefunction, configs))
    eval_ops = EvalOps(
        value=value,
        mc_step=mc_step,
        acceptance_rate=acc_rate,
        placeholder_input=None,
        wavefunction_value=None,
    )
    return eval_ops

  def run_evaluation(self, eval_ops: EvalOps, session, hparams, epoch_num: int) -> List[float]:
    """evaluation.py:113-152: thermalise for num_equilibration_sweeps sweeps, then take
    num_evaluation_samples measurements of the batch-mean local value, num_monte_carlo_sweeps
    sweeps apart.  Each block of num_sites consecutive mc_steps is one persistent-kernel
    launch; the acceptance count the reference computes and drops is kept in
    `self.acceptance_count`."""
    del epoch_num
    steps_per_sweep = hparams.num_sites
    decorrelation = hparams.num_monte_carlo_sweeps * steps_per_sweep
    self.acceptance_count = 0
    fused = _fused_evaluation(eval_ops)
    if fused is not None:
      # the whole loop in ONE host call (vmc_evaluate): batch sums stay on the device, sharded
      # chains are reduced in one float64 all-reduce at the end -- the same list of float32 means
      engine, ensure = fused
      ensure()
      coll = parallel.collective() if parallel.world_size() > 1 else None
      means, accepted = engine.evaluate(coll, hparams.num_equilibration_sweeps * steps_per_sweep,
                                        hparams.num_evaluation_samples, decorrelation)
      self.acceptance_count = accepted
      eval_ops.mc_step.last_accepted = accepted
      return [np.float32(m) for m in means]

    def measurements():
      _run_mc_steps(session, eval_ops.mc_step, hparams.num_equilibration_sweeps * steps_per_sweep)
      for _ in range(hparams.num_evaluation_samples):
        yield session.run(eval_ops.value)
        _run_mc_steps(session, eval_ops.mc_step, decorrelation)
        self.acceptance_count += getattr(eval_ops.mc_step, 'last_accepted', 0)

    return list(measurements())


def _sampling_eval_ops(wavefunction, hparams, shared_resources, make_value) -> EvalOps:
  """The EvalOps of a measurement over the sampler's chains: make_value(engine) is its value tensor, `engine` the one
  that holds the CONFIGS variable mc_step moves."""
  configs = graph_builders.get_configs(shared_resources, hparams.batch_size, hparams.num_sites)
  mc_step, acc_rate = graph_builders.get_monte_carlo_sampling(shared_resources, configs, wavefunction)
  engine = wavefunction._bind(configs)
  return EvalOps(
      value=make_value(engine),
      mc_step=mc_step,
      acceptance_rate=acc_rate,
      placeholder_input=None,
      wavefunction_value=None,
  )


def _sampled(eval_ops, session, hparams, stack, per_sample) -> int:
  """The sample loop of the seven measurement evaluators, on the same schedule as MonteCarloOperatorEvaluator's (which
  keeps its own loop: no all-reduce, and a fused path): thermalises for num_equilibration_sweeps sweeps, then takes
  num_evaluation_samples measurements, num_monte_carlo_sweeps sweeps apart.
  stack(session.run(value)) is the fp64 array of this rank's sums; with sharded chains the ranks' arrays are added by one
  parallel.allreduce_array per sample before per_sample(s, sums) sees them.  Returns the acceptance count."""
  steps_per_sweep = hparams.num_sites
  decorrelation = hparams.num_monte_carlo_sweeps * steps_per_sweep
  sharded = parallel.world_size() > 1
  accepted = 0
  _run_mc_steps(session, eval_ops.mc_step, hparams.num_equilibration_sweeps * steps_per_sweep)
  for s in range(hparams.num_evaluation_samples):
    sums = stack(session.run(eval_ops.value))
    if sharded:
      sums = parallel.allreduce_array(sums)
    per_sample(s, sums)
    _run_mc_steps(session, eval_ops.mc_step, decorrelation)
    accepted += getattr(eval_ops.mc_step, 'last_accepted', 0)
  return accepted


def _std_err(samples):
  """The conventional standard error of the mean over axis 0: std(ddof = 1) / sqrt(n_samples), 0 for a single sample."""
  n = samples.shape[0]
  return samples.std(axis=0, ddof=1) / np.sqrt(n) if n > 1 else np.zeros(samples.shape[1:])


class PairCorrelationTensor(session_lib.Tensor):
  """(zz_sum, ex_sum) [n_pairs] float64 of `pairs` over THIS rank's chains (VmcEngine.pair_correlations);
  `global_batch` is the number of chains of all ranks together."""

  def __init__(self, engine, pairs, which: int, global_batch: int):
    self.engine, self.which, self.global_batch = engine, which, int(global_batch)
    self.pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    super(PairCorrelationTensor, self).__init__(self._value, 'pair_correlations')

  def _value(self):
    return self.engine.pair_correlations(self.pairs, self.which)


class SpinCorrelationEvaluator(WavefunctionEvaluator):
  """<S_i . S_j> by running MCMC (extension: the reference evaluates the energy alone).  The signatures are
  MonteCarloOperatorEvaluator's; `operator` is the list of pairs [(i, j), ...] (None: all N (N - 1) / 2 pairs)."""

  def build_eval_ops(self, wavefunction, operator, hparams,
                     shared_resources: Dict[graph_builders.ResourceName, Any]) -> EvalOps:
    from . import lattice
    pairs = lattice.all_pairs(hparams.num_sites) if operator is None else operator
    return _sampling_eval_ops(wavefunction, hparams, shared_resources, lambda engine: PairCorrelationTensor(
        engine, pairs, wavefunction._which, hparams.batch_size))

  def run_evaluation(self, eval_ops: EvalOps, session, hparams, epoch_num: int) -> Dict[str, np.ndarray]:
    """Thermalises for num_equilibration_sweeps sweeps, then takes num_evaluation_samples measurements,
    num_monte_carlo_sweeps sweeps apart (the loop of MonteCarloOperatorEvaluator).  A measurement is the batch mean,
    over the chains of ALL ranks, of s_i s_j / 4 ('szsz'), of [s_i s_j < 0] psi(swap_ij x) / (2 psi(x)) ('exchange')
    and of their sum ('ss' = S_i . S_j) for every pair: with sharded chains the per-sample fp64 sums of the ranks are
    added by parallel.allreduce_array before the division by the global batch.  Returns a dict: 'pairs' [n_pairs][2];
    for each of the three names the mean over the samples, and under name + '_err' the conventional standard error of
    that mean, std(ddof = 1) / sqrt(n_samples) of the batch means (0 for a single sample); 'samples' [n_samples][3]
    [n_pairs], the batch means themselves."""
    del epoch_num
    value = eval_ops.value
    samples = np.empty((hparams.num_evaluation_samples, 3, value.pairs.shape[0]), np.float64)

    def per_sample(s, sums):                              # [2][n_pairs]: zz, ex
      samples[s, 0] = 0.25 * sums[0] / value.global_batch
      samples[s, 1] = 0.5 * sums[1] / value.global_batch
      samples[s, 2] = (0.25 * sums[0] + 0.5 * sums[1]) / value.global_batch
    self.acceptance_count = _sampled(eval_ops, session, hparams, lambda v: np.stack(v).astype(np.float64), per_sample)
    out = {'pairs': value.pairs.copy(), 'samples': samples}
    for k, name in enumerate(('szsz', 'exchange', 'ss')):
      out[name] = samples[:, k].mean(axis=0)
      out[name + '_err'] = _std_err(samples[:, k])
    return out


class RenyiSwapTensor(session_lib.Tensor):
  """(swap_sum, match_count) [n_regions] float64 of `regions` over THIS rank's chains, paired (c, c + local batch / 2)
  (VmcEngine.renyi2_swap); `masks` [n_regions][num_sites] uint8."""

  def __init__(self, engine, regions, which: int, num_sites: int):
    from . import lattice
    self.engine, self.which = engine, which
    self.masks = lattice.region_masks(regions, num_sites)
    super(RenyiSwapTensor, self).__init__(self._value, 'renyi2_swap')

  def _value(self):
    return self.engine.renyi2_swap(self.masks, self.which)


class RenyiEntropyEvaluator(WavefunctionEvaluator):
  """Second Renyi entanglement entropy S2(A) = -ln Tr rho_A^2 by the replica swap estimator over MCMC chains
  (extension: the reference evaluates the energy alone).  The signatures are MonteCarloOperatorEvaluator's; `operator`
  is the regions -- a [n_regions][num_sites] 0/1 array or a list of site lists (None: lattice.block_regions, the
  blocks [0, l), l = 1 .. N / 2)."""

  def build_eval_ops(self, wavefunction, operator, hparams,
                     shared_resources: Dict[graph_builders.ResourceName, Any]) -> EvalOps:
    from . import lattice
    regions = lattice.block_regions(hparams.num_sites) if operator is None else operator
    return _sampling_eval_ops(wavefunction, hparams, shared_resources, lambda engine: RenyiSwapTensor(
        engine, regions, wavefunction._which, hparams.num_sites))

  def run_evaluation(self, eval_ops: EvalOps, session, hparams, epoch_num: int) -> Dict[str, np.ndarray]:
    """Thermalises for num_equilibration_sweeps sweeps, then takes num_evaluation_samples measurements,
    num_monte_carlo_sweeps sweeps apart (the loop of MonteCarloOperatorEvaluator).  A measurement pairs the chains of
    every rank among themselves, (c, c + local batch / 2): both replicas of a pair live on one rank, and their Philox
    streams are keyed by the global chain id, so they are independent.  With sharded chains the per-sample fp64 swap
    sums, match counts and pair counts of the ranks are added by parallel.allreduce_array before the division.
    Returns a dict: 'regions' [n_regions][num_sites] masks; 'purity' = mean over the samples of swap_sum / pairs;
    'purity_err', the conventional standard error of that mean, std(ddof = 1) / sqrt(n_samples) of the batch means (0
    for a single sample); 's2' = -ln purity; 's2_err' = purity_err / purity; 'match_fraction', the mean share of pairs
    that hold equal magnetisation on the region; 'samples' [n_samples][n_regions], the batch means themselves."""
    del epoch_num
    value = eval_ops.value
    n_regions = value.masks.shape[0]
    samples = np.empty((hparams.num_evaluation_samples, n_regions), np.float64)
    matched = np.empty_like(samples)

    def stack(swap_match):                                # [3][n_regions]: swap sums, match counts, pairs of this rank
      sums = np.empty((3, n_regions), np.float64)
      sums[0], sums[1], sums[2] = swap_match[0], swap_match[1], value.engine.batch_size // 2
      return sums

    def per_sample(s, sums):
      samples[s] = sums[0] / sums[2]
      matched[s] = sums[1] / sums[2]
    self.acceptance_count = _sampled(eval_ops, session, hparams, stack, per_sample)
    purity = samples.mean(axis=0)
    err = _std_err(samples)
    with np.errstate(divide='ignore', invalid='ignore'):
      s2, s2_err = -np.log(purity), err / purity
    return {'regions': value.masks.copy(), 'purity': purity, 'purity_err': err, 's2': s2, 's2_err': s2_err,
            'match_fraction': matched.mean(axis=0), 'samples': samples}


class DimerCorrelationTensor(session_lib.Tensor):
  """(bond_sum [n_bonds], dd_sum [n_pairs]) float64 of `bonds` and of the pairs (a, b) of them over THIS rank's chains
  (VmcEngine.dimer_correlations); `global_batch` is the number of chains of all ranks together."""

  def __init__(self, engine, bonds, pairs, which: int, global_batch: int):
    from . import lattice
    self.engine, self.which, self.global_batch = engine, which, int(global_batch)
    self.bonds = np.ascontiguousarray(np.asarray(bonds, np.int32).reshape(-1, 2))
    self.pairs = lattice.all_bond_pairs(self.bonds.shape[0]) if pairs is None else \
        np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    if self.bonds.shape[0] < 1:
      raise ValueError('dimer correlations need at least one bond')
    if self.pairs.size and (self.pairs.min() < 0 or self.pairs.max() >= self.bonds.shape[0]):
      raise ValueError('a pair names a bond outside 0 .. {}'.format(self.bonds.shape[0] - 1))
    super(DimerCorrelationTensor, self).__init__(self._value, 'dimer_correlations')

  def _value(self):
    return self.engine.dimer_correlations(self.bonds, self.pairs, self.which)


class DimerCorrelationEvaluator(WavefunctionEvaluator):
  """<(S_i . S_j)(S_k . S_l)> by running MCMC (extension: the reference evaluates the energy alone).  The signatures are
  MonteCarloOperatorEvaluator's; `operator` is (bonds, pairs): bonds [(i, j), ...] and pairs [(a, b), ...] of indices
  into them (pairs None: all ordered pairs).  operator None: the Hamiltonian's bonds (`J.txt` of hparams.checkpoint_dir,
  else the periodic chain), each paired with bond 0."""

  def build_eval_ops(self, wavefunction, operator, hparams,
                     shared_resources: Dict[graph_builders.ResourceName, Any]) -> EvalOps:
    from . import lattice
    if operator is None:
      bonds = lattice.load_bonds(getattr(hparams, 'checkpoint_dir', '') or '', hparams.num_sites)
      pairs = [(0, b) for b in range(len(bonds))]
    else:
      bonds, pairs = operator
    return _sampling_eval_ops(wavefunction, hparams, shared_resources, lambda engine: DimerCorrelationTensor(
        engine, bonds, pairs, wavefunction._which, hparams.batch_size))

  def run_evaluation(self, eval_ops: EvalOps, session, hparams, epoch_num: int) -> Dict[str, np.ndarray]:
    """Thermalises for num_equilibration_sweeps sweeps, then takes num_evaluation_samples measurements,
    num_monte_carlo_sweeps sweeps apart (the loop of MonteCarloOperatorEvaluator).  A measurement is the batch mean,
    over the chains of ALL ranks, of the local value of S_i . S_j per bond and of (S_i . S_j)(S_k . S_l) per pair: with
    sharded chains the per-sample fp64 sums of the ranks are added by parallel.allreduce_array before the division by
    the global batch.  Returns a dict: 'bonds' [n_bonds][2]; 'pairs' [n_pairs][2]; 'bond' [n_bonds] = <A>; 'dd' [n_pairs]
    = <A B>; 'connected' [n_pairs] = <A B> - <A><B>, formed per sample from that sample's batch means; under name +
    '_err' the conventional standard error of each mean, std(ddof = 1) / sqrt(n_samples) of the batch means (0 for a
    single sample); 'samples' [n_samples][2][n_pairs], the batch means of dd and connected, and 'bond_samples'
    [n_samples][n_bonds]."""
    del epoch_num
    value = eval_ops.value
    n_bonds, n_pairs = value.bonds.shape[0], value.pairs.shape[0]
    samples = np.empty((hparams.num_evaluation_samples, 2, n_pairs), np.float64)
    bond_samples = np.empty((hparams.num_evaluation_samples, n_bonds), np.float64)

    def per_sample(s, sums):                              # [n_bonds + n_pairs]: bond sums, then dd sums
      bond = sums[:n_bonds] / value.global_batch
      bond_samples[s] = bond
      samples[s, 0] = sums[n_bonds:] / value.global_batch
      samples[s, 1] = samples[s, 0] - bond[value.pairs[:, 0]] * bond[value.pairs[:, 1]]
    self.acceptance_count = _sampled(eval_ops, session, hparams, lambda v: np.concatenate(v).astype(np.float64), per_sample)
    out = {'bonds': value.bonds.copy(), 'pairs': value.pairs.copy(), 'samples': samples, 'bond_samples': bond_samples,
           'bond': bond_samples.mean(axis=0), 'bond_err': _std_err(bond_samples)}
    for k, name in enumerate(('dd', 'connected')):
      out[name] = samples[:, k].mean(axis=0)
      out[name + '_err'] = _std_err(samples[:, k])
    return out


class SymmetryTensor(session_lib.Tensor):
  """ratio_sum [n_ops] float64 of the ops (`perms` [n_ops][num_sites] int32, `flips` [n_ops] uint8) over THIS rank's
  chains (VmcEngine.symmetry_expectations); `global_batch` is the number of chains of all ranks together."""

  def __init__(self, engine, perms, flips, which: int, num_sites: int, global_batch: int):
    from . import lattice
    self.engine, self.which, self.global_batch = engine, which, int(global_batch)
    self.perms, self.flips = lattice.check_symmetry_ops(perms, flips, num_sites)
    super(SymmetryTensor, self).__init__(self._value, 'symmetry_expectations')

  def _value(self):
    return self.engine.symmetry_expectations(self.perms, self.flips, self.which)


class SymmetryEvaluator(WavefunctionEvaluator):
  """<P_g> = <psi(g x) / psi(x)> of site permutations g, optionally followed by the global spin flip, by running MCMC: the
  characters of the state under translations, point-group elements and spin inversion (extension: the reference evaluates
  the energy alone).  The signatures are MonteCarloOperatorEvaluator's; `operator` is (perms, flips) (flips None: no
  flips).  operator None: the translations of the hparams.size_x x hparams.size_y torus (lattice.translations) when
  size_x * size_y = num_sites, otherwise ValueError."""

  def build_eval_ops(self, wavefunction, operator, hparams,
                     shared_resources: Dict[graph_builders.ResourceName, Any]) -> EvalOps:
    from . import lattice
    if operator is None:
      size_x, size_y = getattr(hparams, 'size_x', 0), getattr(hparams, 'size_y', 0)
      if min(size_x, size_y) < 1 or size_x * size_y != hparams.num_sites:
        raise ValueError('SymmetryEvaluator: no ops given and size_x * size_y = {} x {} is not num_sites = {}'.format(
            size_x, size_y, hparams.num_sites))
      perms, flips = lattice.translations(size_x, size_y), None
    else:
      perms, flips = operator
    return _sampling_eval_ops(wavefunction, hparams, shared_resources, lambda engine: SymmetryTensor(
        engine, perms, flips, wavefunction._which, hparams.num_sites, hparams.batch_size))

  def run_evaluation(self, eval_ops: EvalOps, session, hparams, epoch_num: int) -> Dict[str, np.ndarray]:
    """Thermalises for num_equilibration_sweeps sweeps, then takes num_evaluation_samples measurements,
    num_monte_carlo_sweeps sweeps apart (the loop of MonteCarloOperatorEvaluator).  A measurement is the batch mean, over
    the chains of ALL ranks, of psi(g x) / psi(x) per op: with sharded chains the per-sample fp64 sums of the ranks are
    added by parallel.allreduce_array before the division by the global batch.  Returns a dict: 'perms' [n_ops][num_sites];
    'flips' [n_ops]; 'value' [n_ops], the mean over the samples; 'value_err', the conventional standard error of that mean,
    std(ddof = 1) / sqrt(n_samples) of the batch means (0 for a single sample); 'samples' [n_samples][n_ops], the batch
    means themselves."""
    del epoch_num
    value = eval_ops.value
    samples = np.empty((hparams.num_evaluation_samples, value.perms.shape[0]), np.float64)

    def per_sample(s, sums):
      samples[s] = sums / value.global_batch
    self.acceptance_count = _sampled(eval_ops, session, hparams, lambda v: np.asarray(v, np.float64), per_sample)
    return {'perms': value.perms.copy(), 'flips': value.flips.copy(), 'value': samples.mean(axis=0),
            'value_err': _std_err(samples), 'samples': samples}


class ProjectedEnergyTensor(session_lib.Tensor):
  """The sums of VmcEngine.projected_energy over THIS rank's chains for the ops (`perms`, `flips`) and the sectors
  `characters` [n_sectors][n_ops]; `ensure_hamiltonian()` (optional) runs before every measurement: it puts the bonds the
  ops are symmetries of in place."""

  def __init__(self, engine, perms, flips, characters, which: int, num_sites: int, ensure_hamiltonian=None):
    from . import lattice
    self.engine, self.which, self.ensure_hamiltonian = engine, which, ensure_hamiltonian
    self.perms, self.flips = lattice.check_symmetry_ops(perms, flips, num_sites)
    self.characters = lattice.check_characters(characters, self.perms.shape[0])
    super(ProjectedEnergyTensor, self).__init__(self._value, 'projected_energy')

  def _value(self):
    if self.ensure_hamiltonian is not None:
      self.ensure_hamiltonian()
    return self.engine.projected_energy(self.perms, self.flips, self.characters, self.which)


def _ratio_jackknife(num, den):
  """(sum num / sum den, its delete-one-sample jackknife error) over axis 0 of [n_samples][...] arrays; nan where a
  denominator vanishes, error 0 for a single sample (as _std_err)."""
  n = num.shape[0]
  with np.errstate(divide='ignore', invalid='ignore'):
    total_n, total_d = num.sum(axis=0), den.sum(axis=0)
    value = np.where(total_d != 0, total_n / total_d, np.nan)
    if n < 2:
      return value, np.where(np.isnan(value), np.nan, 0.0)
    left_d = total_d - den
    left = np.where(left_d != 0, (total_n - num) / left_d, np.nan)
    err = np.sqrt((n - 1.0) / n * ((left - left.mean(axis=0)) ** 2).sum(axis=0))
  return value, np.where(np.isnan(value), np.nan, err)


class ProjectedEnergyEvaluator(WavefunctionEvaluator):
  """Energies of the symmetry-projected states P_s psi by running MCMC on psi (extension; quantum-number projection as
  post-processing): E_s = <E_loc w_s> / <w_s> with w_s(x) = sum_k chi_s(k) psi(g_k x) / psi(x).  The signatures are
  MonteCarloOperatorEvaluator's; `operator` is (hamiltonian, perms, flips, characters): the HeisenbergHamiltonian whose
  symmetries the ops are, the ops of SymmetryEvaluator and the characters [n_sectors][n_ops] (lattice.sector_characters).
  perms None: the translations of the hparams.size_x x hparams.size_y torus and the characters of its momentum sectors."""

  def build_eval_ops(self, wavefunction, operator, hparams,
                     shared_resources: Dict[graph_builders.ResourceName, Any]) -> EvalOps:
    from . import lattice
    hamiltonian, perms, flips, characters = operator
    if perms is None:
      size_x, size_y = getattr(hparams, 'size_x', 0), getattr(hparams, 'size_y', 0)
      if min(size_x, size_y) < 1 or size_x * size_y != hparams.num_sites:
        raise ValueError('ProjectedEnergyEvaluator: no ops given and size_x * size_y = {} x {} is not num_sites = {}'.format(
            size_x, size_y, hparams.num_sites))
      perms, flips = lattice.translations(size_x, size_y), None
      characters = lattice.sector_characters(size_x, size_y, False)[1]
    configs = graph_builders.get_configs(shared_resources, hparams.batch_size, hparams.num_sites)
    ensure = None if configs is None else (lambda: configs._ensure_hamiltonian(hamiltonian))
    return _sampling_eval_ops(wavefunction, hparams, shared_resources, lambda engine: ProjectedEnergyTensor(
        engine, perms, flips, characters, wavefunction._which, hparams.num_sites, ensure))

  def run_evaluation(self, eval_ops: EvalOps, session, hparams, epoch_num: int) -> Dict[str, np.ndarray]:
    """Thermalises for num_equilibration_sweeps sweeps, then takes num_evaluation_samples measurements,
    num_monte_carlo_sweeps sweeps apart (the loop of MonteCarloOperatorEvaluator).  A measurement is the stacked sums
    [w_sum (n_sectors), we_sum (n_sectors), e_sum, n_alive] over the chains of ALL ranks: with sharded chains the ranks'
    fp64 arrays are added by one parallel.allreduce_array per sample.  With W_t, WE_t, E_t, A_t the sums of sample t,
    returns a dict: 'energy' [n_sectors] = sum_t WE_t / sum_t W_t and 'energy_err', the delete-one-sample jackknife error
    of that ratio; 'weight' = sum_t W_t / sum_t A_t and 'weight_err', the standard error of the per-sample weights
    W_t / A_t; 'plain_energy' = sum_t E_t / sum_t A_t, the unprojected energy, and 'plain_energy_err', the standard error
    of E_t / A_t; 'samples' [n_samples][2 n_sectors + 2], the stacked sums themselves; 'perms', 'flips', 'characters'.
    A sector whose sum_t W_t is exactly 0 has energy nan (no exception); a single sample gives the errors 0."""
    del epoch_num
    value = eval_ops.value
    n_s = value.characters.shape[0]
    samples = np.empty((hparams.num_evaluation_samples, 2 * n_s + 2), np.float64)

    def stack(v):
      return np.concatenate([np.asarray(v['w_sum'], np.float64), np.asarray(v['we_sum'], np.float64),
                             np.array([v['e_sum'], v['n_alive']], np.float64)])

    def per_sample(s, sums):
      samples[s] = sums
    self.acceptance_count = _sampled(eval_ops, session, hparams, stack, per_sample)
    w, we, e, alive = samples[:, :n_s], samples[:, n_s:2 * n_s], samples[:, 2 * n_s], samples[:, 2 * n_s + 1]
    energy, energy_err = _ratio_jackknife(we, w)
    with np.errstate(divide='ignore', invalid='ignore'):
      weight = w.sum(axis=0) / alive.sum()
      weight_err = _std_err(w / alive[:, None])
      plain = e.sum() / alive.sum()
      plain_err = _std_err((e / alive)[:, None])[0]
    return {'perms': value.perms.copy(), 'flips': value.flips.copy(), 'characters': value.characters.copy(),
            'energy': energy, 'energy_err': energy_err, 'weight': weight, 'weight_err': weight_err,
            'plain_energy': float(plain), 'plain_energy_err': float(plain_err), 'samples': samples}


class EnergyMomentsTensor(session_lib.Tensor):
  """The six sums of VmcEngine.energy_moments over THIS rank's chains, float64 [6]: e, e^2, g, e g, g^2, chains alive;
  `ensure_hamiltonian()` (optional) runs before every measurement: it puts the Hamiltonian's bonds in place."""

  def __init__(self, engine, which: int, ensure_hamiltonian=None):
    self.engine, self.which, self.ensure_hamiltonian = engine, which, ensure_hamiltonian
    self.last_rows2 = 0
    super(EnergyMomentsTensor, self).__init__(self._value, 'energy_moments')

  def _value(self):
    if self.ensure_hamiltonian is not None:
      self.ensure_hamiltonian()
    v = self.engine.energy_moments(self.which)
    self.last_rows2 = v['n_rows2']
    return np.array([v['e_sum'], v['e2_sum'], v['g_sum'], v['eg_sum'], v['g2_sum'], v['n_alive']], np.float64)


LANCZOS_QUANTITIES = ('energy', 'variance', 'lanczos_energy', 'alpha', 'lanczos_variance', 'extrapolated_energy',
                      'h2_check', 'h1', 'h2', 'h3', 'h4')
# The local energies are fp32: a variance below this share of <e^2> is below what they resolve (eps32^2 ~ 1.4e-14 times the
# conditioning of a sum of ratios), and the overlap matrix of the Lanczos step counts as degenerate.
LANCZOS_DEGENERATE = 1e-10


def lanczos_step(sums) -> Dict[str, float]:
  """The quantities of LANCZOS_QUANTITIES from summed sums [6] = (sum e, sum e^2, sum g, sum e g, sum g^2, chains alive).
  h1 .. h4 = <e>, <e^2>, <e g>, <g^2>; h2 = <e^2> serves both matrices of
    [[h1, h2], [h2, h3]] v = E [[1, h1], [h1, h2]] v,
  so the overlap matrix is a Gram matrix of the samples; lanczos_energy is the lowest E -- the lower root of
  var E^2 - (h3 - h1 h2) E + (h1 h3 - h2^2) = 0, var = h2 - h1^2, taken in its cancellation-free form -- alpha = v1 / v0,
  lanczos_variance = (h2 + 2 alpha h3 + alpha^2 h4) / (1 + 2 alpha h1 + alpha^2 h2) - E1^2, and extrapolated_energy the
  line through (var, h1) and (lanczos_variance, E1) at variance 0.  A degenerate overlap matrix (var <= LANCZOS_DEGENERATE
  h2: an eigenstate) gives lanczos_energy = extrapolated_energy = energy, alpha = 0, lanczos_variance = variance; no
  chain alive gives nan throughout."""
  s = np.asarray(sums, np.float64)
  if not s[5] > 0:
    return {k: float('nan') for k in LANCZOS_QUANTITIES}
  h1, h2, hg, h3, h4 = (float(v) for v in s[:5] / s[5])
  var = h2 - h1 * h1
  out = {'energy': h1, 'variance': var, 'h2_check': hg, 'h1': h1, 'h2': h2, 'h3': h3, 'h4': h4}
  e1, alpha, var1 = h1, 0.0, var
  if var > LANCZOS_DEGENERATE * h2:
    p, q = h3 - h1 * h2, h1 * h3 - h2 * h2
    t = p + np.copysign(np.sqrt(max(p * p - 4.0 * var * q, 0.0)), p)
    roots = [t / (2.0 * var)] + ([2.0 * q / t] if t != 0 else [])
    e1 = float(min(roots))
    d0 = h2 - e1 * h1                                   # the first row of (A - E B) v = 0
    alpha = float((e1 - h1) / d0) if d0 != 0 else float('inf')
    norm = 1.0 + 2.0 * alpha * h1 + alpha * alpha * h2
    if np.isfinite(alpha) and norm > 0:
      var1 = (h2 + 2.0 * alpha * h3 + alpha * alpha * h4) / norm - e1 * e1
    else:
      e1, alpha, var1 = h1, 0.0, var
  out['lanczos_energy'], out['alpha'], out['lanczos_variance'] = e1, alpha, var1
  out['extrapolated_energy'] = e1 if var1 == var else h1 - var * (e1 - h1) / (var1 - var)
  return out


def _jackknife(samples, fn, names):
  """({name: fn(sum of the samples)[name]}, {name: delete-one-sample jackknife error}); errors 0 for a single sample.
  The deviations are taken against the first leave-one-out value, so identical samples give exactly 0."""
  n = samples.shape[0]
  total = samples.sum(axis=0)
  value = fn(total)
  err = {k: 0.0 for k in names}
  if n > 1:
    left = [fn(total - samples[i]) for i in range(n)]
    for k in names:
      d = np.array([l[k] - left[0][k] for l in left], np.float64)
      err[k] = float(np.sqrt((n - 1.0) / n * ((d - d.mean()) ** 2).sum()))
  return value, err


class LanczosStepEvaluator(WavefunctionEvaluator):
  """One Lanczos step and the variance extrapolation by running MCMC on psi (extension): from the local values e of H and
  g of H^2 per chain, the moments <H^n>, n = 1 .. 4, the best energy of psi + alpha H psi, its variance, and the energy
  extrapolated to zero variance through the two points.  The signatures are MonteCarloOperatorEvaluator's; `operator` is
  the HeisenbergHamiltonian."""

  def build_eval_ops(self, wavefunction, operator, hparams,
                     shared_resources: Dict[graph_builders.ResourceName, Any]) -> EvalOps:
    configs = graph_builders.get_configs(shared_resources, hparams.batch_size, hparams.num_sites)
    ensure = None if configs is None else (lambda: configs._ensure_hamiltonian(operator))
    return _sampling_eval_ops(wavefunction, hparams, shared_resources, lambda engine: EnergyMomentsTensor(
        engine, wavefunction._which, ensure))

  def run_evaluation(self, eval_ops: EvalOps, session, hparams, epoch_num: int) -> Dict[str, Any]:
    """Thermalises for num_equilibration_sweeps sweeps, then takes num_evaluation_samples measurements,
    num_monte_carlo_sweeps sweeps apart (the loop of MonteCarloOperatorEvaluator).  A measurement is the six sums of
    VmcEngine.energy_moments over the chains of ALL ranks: with sharded chains the ranks' fp64 arrays are added by one
    parallel.allreduce_array per sample.  Returns a dict: every name of LANCZOS_QUANTITIES, formed by lanczos_step from the
    sums of all samples, and under name + '_err' its delete-one-sample jackknife error (0 for a single sample);
    'n_rows2', the length of the last measurement's second-order list on this rank; 'samples' [n_samples][6], the
    stacked sums."""
    del epoch_num
    value = eval_ops.value
    samples = np.empty((hparams.num_evaluation_samples, 6), np.float64)

    def per_sample(s, sums):
      samples[s] = sums
    self.acceptance_count = _sampled(eval_ops, session, hparams, lambda v: np.asarray(v, np.float64), per_sample)
    out, err = _jackknife(samples, lanczos_step, LANCZOS_QUANTITIES)
    out = dict(out)
    for k in LANCZOS_QUANTITIES:
      out[k + '_err'] = err[k] if np.isfinite(out[k]) else float('nan')
    out['samples'] = samples
    out['n_rows2'] = int(getattr(value, 'last_rows2', 0))
    return out


class OverlapTensor(session_lib.Tensor):
  """The four sums of VmcEngine.overlap over THIS rank's chains, float64 [4]: s1, s2, chains alive, log_scale (s1 and s2
  are in units of exp(log_scale) and exp(2 log_scale))."""

  def __init__(self, engine):
    self.engine = engine
    super(OverlapTensor, self).__init__(self._value, 'overlap')

  def _value(self):
    v = self.engine.overlap()
    return np.array([v['s1'], v['s2'], v['alive'], v['log_scale']], np.float64)


def fidelity_from_sums(s1, s2, alive) -> float:
  """s1^2 / (alive s2), the estimator of |<phi|psi>|^2 / (<psi|psi><phi|phi>) from sums at ONE scale; 0 -- never nan --
  when s2 = 0 (phi vanishes on every chain) or no chain is alive."""
  s1, s2, alive = float(s1), float(s2), float(alive)
  if not s2 > 0 or not alive > 0:
    return 0.0
  return s1 * s1 / (alive * s2)


def overlap_common_scale(samples):
  """[n_samples][3] = s1, s2, alive of `samples` [n_samples][4] (s1, s2, alive, log_scale) at the largest log_scale among
  the samples that hold a ratio (s2 > 0), in fp64: s1 exp(l - L), s2 exp(2 (l - L)).  A sample far below the common scale
  underflows to 0, which is its share of the sums."""
  samples = np.asarray(samples, np.float64).reshape(-1, 4)
  out = samples[:, :3].copy()
  live = samples[:, 1] > 0
  if live.any():
    shift = np.where(live, samples[:, 3] - samples[live, 3].max(), 0.0)
    with np.errstate(under='ignore'):
      out[:, 0] = samples[:, 0] * np.exp(shift)
      out[:, 1] = samples[:, 1] * np.exp(2.0 * shift)
  return out


class OverlapEvaluator(WavefunctionEvaluator):
  """Fidelity of psi with a second, frozen state phi of the same architecture by running MCMC on psi (extension):
  F = |<phi|psi>|^2 / (<psi|psi><phi|phi>) = <r>^2 / <r^2>, r = phi / psi on chains drawn from |psi|^2.  The signatures are
  MonteCarloOperatorEvaluator's; `operator` is phi, a wavefunction built like psi that holds its values (or receives them
  before run_evaluation); it is bound to the chains' second parameter set.  One rank only."""

  def build_eval_ops(self, wavefunction, operator, hparams,
                     shared_resources: Dict[graph_builders.ResourceName, Any]) -> EvalOps:
    if parallel.is_distributed():
      raise NotImplementedError('OverlapEvaluator runs on one rank (the sums of two ranks have no common scale)')
    if operator is None or operator is wavefunction:
      raise ValueError('OverlapEvaluator: `operator` is the second wavefunction')

    def make_value(engine):
      configs = graph_builders.get_configs(shared_resources, hparams.batch_size, hparams.num_sites)
      if operator._bind(configs) is not engine or operator._which != 1:
        raise ValueError('OverlapEvaluator: the second wavefunction must take the frozen parameter set of psi\'s chains')
      return OverlapTensor(engine)
    return _sampling_eval_ops(wavefunction, hparams, shared_resources, make_value)

  def run_evaluation(self, eval_ops: EvalOps, session, hparams, epoch_num: int) -> Dict[str, Any]:
    """Thermalises for num_equilibration_sweeps sweeps, then takes num_evaluation_samples measurements,
    num_monte_carlo_sweeps sweeps apart (the loop of MonteCarloOperatorEvaluator).  A measurement is the four sums of
    VmcEngine.overlap; the samples are brought to one scale on the host in fp64 (overlap_common_scale).  With S1_t, S2_t,
    A_t the scaled sums of sample t, returns a dict: 'fidelity' = (sum_t S1_t)^2 / (sum_t A_t sum_t S2_t) and
    'fidelity_err', its delete-one-sample jackknife error (0 for a single sample); 'overlap_sign', the sign of sum_t S1_t;
    'alive_fraction' = sum_t A_t / (n_samples batch_size); 'samples' [n_samples][4], the sums as measured.  A phi that
    vanishes on every chain gives fidelity 0, never nan."""
    del epoch_num
    samples = np.empty((hparams.num_evaluation_samples, 4), np.float64)

    def per_sample(s, sums):
      samples[s] = sums
    self.acceptance_count = _sampled(eval_ops, session, hparams, lambda v: np.asarray(v, np.float64), per_sample)
    scaled = overlap_common_scale(samples)
    n = scaled.shape[0]
    total = scaled.sum(axis=0)
    err = 0.0
    if n > 1:
      left = np.array([fidelity_from_sums(*(total - scaled[t])) for t in range(n)], np.float64)
      err = float(np.sqrt((n - 1.0) / n * ((left - left.mean()) ** 2).sum()))
    chains = float(n) * float(hparams.batch_size)
    return {'fidelity': fidelity_from_sums(*total), 'fidelity_err': err, 'overlap_sign': float(np.sign(total[0])),
            'alive_fraction': float(total[2] / chains) if chains > 0 else 0.0, 'samples': samples}


class VectorWavefunctionEvaluator(WavefunctionEvaluator):
  """evaluation.py:155-246: dumps psi over a basis file.  Offline tool outside the hot path
  (SURVEY.md 2); `Wavefunction.__call__` on an array gives the same amplitudes."""

  def build_eval_ops(self, wavefunction, operator, hparams, shared_resources):
    raise NotImplementedError('VectorWavefunctionEvaluator is outside the MI355X hot path')

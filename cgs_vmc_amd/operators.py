"""Operator interface and the Heisenberg Hamiltonian (mirror of cgs_vmc/operators.py).

The arithmetic of HeisenbergHamiltonian.build / local_value / apply_in_place runs in
libcgsvmc_hip.so: k_bond_count / k_bond_fill list the antiparallel bonds of every chain,
k_tail16 evaluates psi(swap_ij R)/psi(R) for exactly those rows and k_eloc_reduce sums them
per chain.  The results equal the reference's "evaluate every bond, then mask"
(operators.py:166-168) because masked rows contribute exactly zero.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import session as session_lib


class Operator():
  """Operators base class (operators.py:13-87)."""

  def build(self, wavefunction, inputs, psi=None):
    raise NotImplementedError

  def local_value(self, wavefunction, inputs, psi=None):
    raise NotImplementedError

  def apply_in_place(self, wavefunction, inputs, psi=None):
    raise NotImplementedError

  def apply(self, wavefunction):
    raise NotImplementedError


class HeisenbergHamiltonian(Operator):
  """sum over bonds of S_i.S_j with couplings j_x (transverse) and j_z
  (operators.py:212-287).  `j_x` / `j_z` may also be per-bond sequences (extension; the
  reference takes one value for all bonds, operators.py:215-225)."""

  def __init__(self, bonds: List[Tuple[int, int]], j_x, j_z):
    self._bonds_list = [(int(b[0]), int(b[1])) for b in bonds]
    nb = len(self._bonds_list)
    self._j_x = np.broadcast_to(np.asarray(j_x, np.float32), (nb,)).copy()
    self._j_z = np.broadcast_to(np.asarray(j_z, np.float32), (nb,)).copy()

  def _engine_for(self, wavefunction, inputs):
    from . import graph_builders
    if not isinstance(inputs, graph_builders.ConfigsVariable):
      raise TypeError('the MI355X Hamiltonian kernels act on the CONFIGS variable '
                      '(graph_builders.get_configs)')
    engine = wavefunction._bind(inputs)
    inputs._ensure_hamiltonian(self)
    return engine

  def build(self, wavefunction, inputs, psi=None) -> Tuple[session_lib.Tensor, ...]:
    """(diagonal matrix element, off-diagonal term sum_bonds 0.5 jx [s_i s_j<0] psi(R_ij)),
    operators.py:227-247."""
    del psi
    engine = self._engine_for(wavefunction, inputs)

    def diag():
      inputs._ensure_hamiltonian(self)      # another operator may have been evaluated in between
      return engine.local_energy_terms(wavefunction._which)[0]

    def offdiag():
      inputs._ensure_hamiltonian(self)
      d, o = engine.local_energy_terms(wavefunction._which)
      return o * engine.amplitude(None, wavefunction._which)[1]
    return session_lib.Tensor(diag, 'sz_elements'), session_lib.Tensor(offdiag, 's_perp_terms')

  def local_value(self, wavefunction, inputs, psi=None) -> session_lib.Tensor:
    """diag + s_perp / psi (operators.py:249-259)."""
    del psi
    engine = self._engine_for(wavefunction, inputs)
    return LocalValueTensor(self, wavefunction, inputs, engine)

  def apply_in_place(self, wavefunction, inputs, psi=None) -> session_lib.Tensor:
    """diag * psi + s_perp (operators.py:261-271)."""
    del psi
    engine = self._engine_for(wavefunction, inputs)

    def value():
      inputs._ensure_hamiltonian(self)
      eloc, _ = engine.local_energy(wavefunction._which)
      return eloc * engine.amplitude(None, wavefunction._which)[1]
    return session_lib.Tensor(value, 'h_psi')

  def apply(self, wavefunction):
    raise NotImplementedError('TransformedWavefunction (operators.py:90-125) is used by no '
                              'driver and is outside the MI355X hot path')


class JQHamiltonian(HeisenbergHamiltonian):
  """The Heisenberg Hamiltonian of `bonds` plus four-spin terms (extension, no reference counterpart):
    H = sum_bonds S_i.S_j  -  sum_t q_t (1/4 - S_i.S_j)(1/4 - S_k.S_l),   t = (i, j, k, l) four distinct sites,
  the J-Q model for the terms of lattice.jq_chain_terms / jq_torus_terms.  `q` is a scalar or one value per term.
  `exchange_sign` is the sign the transverse part of the projectors carries: +1 in the physical frame, -1 in the
  sublattice-rotated frame that goes with j_x < 0; it defaults to the common sign of `j_x` (ValueError where the bonds
  disagree or every j_x is 0).  Installing it on the chains uploads the bonds and then the terms
  (ConfigsVariable._ensure_hamiltonian); installing a plain HeisenbergHamiltonian afterwards clears them.  Every local
  energy -- evaluation, the gradient modes, the SR right-hand side -- is then that of the whole Hamiltonian
  (csrc/fourspin.hip)."""

  def __init__(self, bonds, j_x, j_z, four_spin_terms, q, exchange_sign=None):
    super(JQHamiltonian, self).__init__(bonds, j_x, j_z)
    from . import lattice
    self._four_spin_terms = lattice.check_four_spin_terms(four_spin_terms)
    n_terms = self._four_spin_terms.shape[0]
    q = np.asarray(q, np.float32)
    if q.ndim > 1 or (q.ndim == 1 and q.shape[0] != n_terms):
      raise ValueError('JQHamiltonian: q is a scalar or one value per term ({} terms), got shape {}'.format(n_terms, q.shape))
    self._q = np.broadcast_to(q, (n_terms,)).copy()
    if not np.all(np.isfinite(self._q)):
      raise ValueError('JQHamiltonian: every q must be finite')
    if exchange_sign is None:
      signs = set(np.sign(self._j_x).astype(int).tolist())
      if signs not in ({1}, {-1}):
        raise ValueError('JQHamiltonian: the bonds do not share one sign of j_x ({}); state exchange_sign = +1 (physical '
                         'frame) or -1 (sublattice-rotated frame)'.format(sorted(signs)))
      exchange_sign = signs.pop()
    if exchange_sign not in (1, -1):
      raise ValueError('JQHamiltonian: exchange_sign is +1 or -1, got {!r}'.format(exchange_sign))
    self._exchange_sign = int(exchange_sign)


class HeisenbergBond(HeisenbergHamiltonian):
  """S_i . S_j on one bond (operators.py:128-169): `build` returns
  (0.25 j_z s_i s_j, 0.25 j_x 2 [s_i s_j < 0] psi(R with i and j exchanged)).  It is the
  one-bond case of the Hamiltonian kernels (the connected-row list then has at most one row per
  chain)."""

  def __init__(self, bond: Tuple[int, int], j_x, j_z):
    super(HeisenbergBond, self).__init__([bond], j_x, j_z)
    self._bond = (int(bond[0]), int(bond[1]))


class LocalValueTensor(session_lib.Tensor):
  """E_loc[B] of `operator` under `wavefunction` on the chains."""

  def __init__(self, operator, wavefunction, configs, engine):
    self.operator, self.wavefunction, self.configs, self.engine = (
        operator, wavefunction, configs, engine)
    super(LocalValueTensor, self).__init__(self._value, 'local_value')

  def _value(self):
    self.configs._ensure_hamiltonian(self.operator)
    return self.engine.local_energy(self.wavefunction._which)[0]

  def mean(self) -> float:
    """Batch mean over ALL ranks' chains (evaluation.py:102 tf.reduce_mean)."""
    from . import parallel
    self.configs._ensure_hamiltonian(self.operator)
    _, m = self.engine.local_energy(self.wavefunction._which, want_eloc=False)
    if parallel.world_size() > 1:
      m = parallel.allreduce_sum(m) / parallel.world_size()
    return m


def reduce_mean(tensor) -> session_lib.Tensor:
  """tf.reduce_mean for the tensors of this module."""
  if isinstance(tensor, LocalValueTensor):
    out = session_lib.Tensor(lambda: np.float32(tensor.mean()), 'mean')
    out.local_value_tensor = tensor       # evaluation.run_evaluation fuses the loop over it
    return out
  return session_lib.Tensor(lambda: np.float32(np.mean(tensor._run())), 'mean')

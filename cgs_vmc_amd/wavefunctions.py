"""Wavefunction interface and the fully-connected ansatz (mirror of
cgs_vmc/wavefunctions.py, hot-path scope: SURVEY.md 8a rows a6-a10).

A `Wavefunction` is a host-side description (shape, activations, parameter vector).  The
arithmetic runs in libcgsvmc_hip.so: applying a wavefunction to the CONFIGS variable of
graph_builders binds it to that variable's `VmcEngine` as parameter set psi (the first
wavefunction bound) or omega (its deep copy, the LogOverlapITSWO supervisor).
"""
from __future__ import annotations

import copy
import inspect
import os
from typing import Any, Dict, List, Optional

import numpy as np

from . import _hip
from . import layers
from . import session as session_lib

_name_counts: Dict[str, int] = {}
_init_counter = [0]


def _init_count() -> int:
  _init_counter[0] += 1
  return _init_counter[0] - 1


def _unique_name(name: str) -> str:
  """Sonnet module name uniquification: name, name_1, name_2, ..."""
  n = _name_counts.get(name, 0)
  _name_counts[name] = n + 1
  return name if n == 0 else '%s_%d' % (name, n)


def reset_name_scope():
  _name_counts.clear()
  _init_counter[0] = 0


class Wavefunction:
  """Wavefunction interface (wavefunctions.py:21-297)."""

  def __init__(self, name: str = 'wavefunction'):
    self._name = name
    self._unique_name = _unique_name(name)
    self._sub_wavefunctions: List['Wavefunction'] = []
    self._exp_norm_shift = None
    self._engine = None
    self._which = None

  # -- graph connection ----------------------------------------------------
  def __call__(self, inputs) -> session_lib.Tensor:
    return self._build(inputs)

  def _build(self, inputs):
    raise NotImplementedError

  def __add__(self, other):
    raise NotImplementedError('sum/diff/prod composites are outside the MI355X hot path '
                              '(SURVEY.md 2: composites OUT OF SCOPE)')

  __sub__ = __add__

  def __mul__(self, other):
    """wavefunctions.py:107-161: psi_a(x) psi_b(x) as one wavefunction over one set of chains.  Scalar factors (a float
    or a session.Tensor) are out of scope."""
    if isinstance(other, Wavefunction):
      return ProductOfWavefunctions(self, other)
    raise NotImplementedError('a product with a scalar factor (%s) is outside the MI355X hot path; only '
                              'wavefunction * wavefunction has HIP kernels' % type(other).__name__)

  def get_trainable_variables(self) -> List[session_lib.Variable]:
    """wavefunctions.py:167-175: own variables in creation order, then sub-wavefunctions'."""
    variables = list(self._own_variables())
    for sub in self._sub_wavefunctions:
      variables += sub.get_trainable_variables()
    return variables

  def _own_variables(self):
    return []

  def __deepcopy__(self, memo: Dict[int, Any]) -> 'Wavefunction':
    """wavefunctions.py:177-204: a twin built from the same constructor arguments (deep-copied,
    so sub-wavefunctions get twins too) with fresh variables under the name dc_<name>."""
    twin = memo.get(id(self))
    if twin is None:
      ctor = inspect.signature(type(self).__init__).parameters
      kwargs = {arg: copy.deepcopy(getattr(self, '_' + arg), memo)
                for arg in ctor if arg not in ('self', 'name')}
      twin = type(self)(name='dc_' + self._unique_name, **kwargs)
      memo[id(self)] = twin
    return twin

  # -- normalisation -------------------------------------------------------
  def add_exp_normalization(self, initial_exp_norm_shift: float = -10.):
    """wavefunctions.py:206-232: non-trainable scalar shift, psi = exp(logit - shift)."""
    self._exp_norm_shift = np.float32(initial_exp_norm_shift)

  def normalize_batch(self, batch_of_amplitudes, max_value: float = 1e10):
    """wavefunctions.py:234-259."""
    if self._exp_norm_shift is None:
      return None

    def run():
      log_max = self._global_log_max(batch_of_amplitudes)
      if log_max is None:        # no psi > 0 anywhere (signed amplitudes): the shift is kept
        return
      self._set_shift(np.float32(self._get_shift() + (log_max - np.log(np.float32(max_value)))))
    return session_lib.Op(run, 'normalize_batch')

  def _global_log_max(self, batch_of_amplitudes) -> np.float32:
    """log(max_b psi_b) over ALL ranks (wavefunctions.py:250, 283).  For this ansatz's own
    amplitudes the max is taken over the logits and `log(exp(max_logit - shift))` is evaluated
    once, as vmc_update_norm does: where psi overflows float32 the reference's value is inf;
    the logit-domain value max_logit - shift is used there, on every path (single GPU, sharded,
    op-by-op), so that sharded and unsharded runs agree."""
    from . import parallel
    own = (isinstance(batch_of_amplitudes, AmplitudeTensor)
           and batch_of_amplitudes.wavefunction is self and self._exp_norm_shift is not None)
    if own:
      top = np.float32(parallel.allreduce_max(float(np.max(batch_of_amplitudes.logits()))))
      gap = np.float32(top - np.float32(self._get_shift()))
      with np.errstate(over='ignore'):
        psi_max = np.exp(gap, dtype=np.float32)
      if np.isfinite(psi_max) and psi_max > 0:
        return np.float32(np.log(psi_max))
      return gap
    psi = np.asarray(batch_of_amplitudes._run())
    with np.errstate(divide='ignore'):
      return np.float32(np.log(np.float32(parallel.allreduce_max(float(np.max(psi))))))

  def update_norm(self, batch_of_amplitudes, max_value: float = 1e10):
    """wavefunctions.py:261-288."""
    if self._exp_norm_shift is None:
      return None
    return session_lib.Op(lambda: self._update_norm(batch_of_amplitudes, max_value),
                          'update_norm')

  def _update_norm(self, batch_of_amplitudes, max_value):
    raise NotImplementedError

  def _get_shift(self):
    return self._exp_norm_shift

  def _set_shift(self, value):
    self._exp_norm_shift = np.float32(value)

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    raise NotImplementedError


def module_transfer_ops(source_module: Wavefunction, target_module: Wavefunction) -> session_lib.Op:
  """wavefunctions.py:300-325: assign every trainable variable of source to target."""
  def run():
    if (source_module._engine is not None and source_module._engine is target_module._engine
        and source_module._which == _hip.VMC_PSI and target_module._which == _hip.VMC_OMEGA):
      source_module._engine.transfer_params()          # device-to-device (a product: both factors)
      target_module._has_values, target_module._theta = True, None
      return
    src = source_module.get_trainable_variables()
    dst = target_module.get_trainable_variables()
    for s, t in zip(src, dst):
      t.load(s.eval())
  return session_lib.Op(run, 'module_transfer')


class FullyConnectedNetwork(Wavefunction):
  """[Linear(layer_size), nonlinearity] x num_layers -> Linear(1) -> squeeze ->
  (- exp_norm_shift) -> exp   (wavefunctions.py:328-388)."""
  _ansatz = 'fully_connected'     # engine kernel family (include/cgsvmc.h VMC_ANSATZ_*)

  def __init__(self, num_layers: int, layer_size: int,
               nonlinearity=layers.NONLINEARITIES['relu'],
               output_activation=layers.NONLINEARITIES['exp'],
               name: str = 'fully_connected_network'):
    super(FullyConnectedNetwork, self).__init__(name=name)
    self._num_layers = num_layers
    self._layer_size = layer_size
    self._nonlinearity = nonlinearity
    self._output_activation = output_activation
    if output_activation == layers.NONLINEARITIES['exp']:
      self.add_exp_normalization()
    self._n_sites: Optional[int] = None
    self._theta: Optional[np.ndarray] = None     # host copy until bound to an engine
    self._has_values = False                     # variables initialised / restored
    session_lib.get_default_graph().global_initializers.append(self._maybe_initialize)

  # -- parameters ----------------------------------------------------------
  def _shapes(self):
    shapes, names = [], []
    fan_in = self._n_sites
    for l in range(self._num_layers + 1):
      out = self._layer_size if l < self._num_layers else 1
      lin = 'linear' if l == 0 else 'linear_%d' % l
      names += ['%s/%s/w' % (self._unique_name, lin), '%s/%s/b' % (self._unique_name, lin)]
      shapes += [(fan_in, out), (out,)]
      fan_in = out
    return names, shapes

  @property
  def num_params(self) -> int:
    return int(sum(int(np.prod(s)) for s in self._shapes()[1]))

  def _maybe_initialize(self):
    if self._n_sites is not None and self._get_theta(allow_none=True) is None:
      # unseeded like the reference unless CGS_VMC_INIT_SEED is set (tests, reproducible runs)
      seed = os.environ.get('CGS_VMC_INIT_SEED')
      self.initialize(None if seed is None else int(seed) + _init_count())

  def initialize(self, seed=None):
    """snt.Linear defaults: w ~ truncated normal(sigma = 1/sqrt(fan_in)), b = 0."""
    if self._n_sites is None:
      raise ValueError('wavefunction is not connected to inputs yet')
    rng = np.random.default_rng(seed)
    parts = []
    for shp in self._shapes()[1]:
      if len(shp) == 2:
        w = rng.standard_normal(shp)
        bad = np.abs(w) > 2
        while bad.any():
          w[bad] = rng.standard_normal(int(bad.sum()))
          bad = np.abs(w) > 2
        parts.append((w / np.sqrt(shp[0])).ravel())
      else:
        parts.append(np.zeros(shp).ravel())
    self._set_theta(np.concatenate(parts).astype(np.float32))

  def _get_theta(self, allow_none=False):
    if not self._has_values:
      if allow_none:
        return None
      raise ValueError('Attempting to use uninitialized variables of %s' % self._unique_name)
    if self._engine is not None and self._theta is None:
      return self._engine.get_params(self._which)
    return self._theta

  def _set_theta(self, theta):
    theta = np.ascontiguousarray(theta, np.float32)
    self._has_values = True
    if self._engine is not None:
      self._engine.set_params(theta, self._which)
      self._theta = None          # the device copy is authoritative from now on
    else:
      self._theta = theta

  def _own_variables(self):
    if self._n_sites is None:
      raise ValueError('wavefunction %s has no variables before it is connected to inputs'
                       % self._unique_name)
    names, shapes = self._shapes()
    out, off = [], 0
    for name, shp in zip(names, shapes):
      n = int(np.prod(shp))

      def getter(off=off, n=n):
        return self._get_theta()[off:off + n]

      def setter(value, off=off, n=n):
        theta = self._get_theta(allow_none=True)
        if theta is None:
          theta = np.zeros(self.num_params, np.float32)
        theta = theta.copy()
        theta[off:off + n] = np.asarray(value, np.float32).ravel()
        self._set_theta(theta)

      out.append(session_lib.Variable(name, shp, getter, setter, trainable=True))
      off += n
    return out

  # -- engine binding ------------------------------------------------------
  def _engine_spec(self):
    """Keyword arguments that describe this ansatz to VmcEngine / vmc_create."""
    return dict(ansatz=self._ansatz, num_layers=self._num_layers, layer_size=self._layer_size,
                nonlinearity=self._nonlinearity.name,
                output_activation=self._output_activation.name)

  def _bind(self, configs_var):
    """Connects this ansatz to the engine that owns `configs_var`."""
    n_sites = configs_var.shape[1]
    if self._n_sites is not None and self._n_sites != n_sites:
      raise ValueError('Input tensor has wrong shape.')
    self._n_sites = n_sites
    engine = configs_var._get_engine(self)
    if self._engine is engine:
      return engine
    if self._engine is not None:
      raise ValueError('wavefunction %s is already bound to another CONFIGS variable'
                       % self._unique_name)
    which = configs_var._claim_slot(self)
    host_theta = self._theta
    self._engine, self._which = engine, which
    if host_theta is not None:
      engine.set_params(host_theta, which)
      self._theta = None
    if self._exp_norm_shift is not None:
      engine.set_shift(float(self._exp_norm_shift), which)
    return engine

  def _get_shift(self):
    if self._engine is not None:
      return np.float32(self._engine.get_shift(self._which))
    return self._exp_norm_shift

  def _set_shift(self, value):
    self._exp_norm_shift = np.float32(value)
    if self._engine is not None:
      self._engine.set_shift(float(value), self._which)

  def _build(self, inputs) -> session_lib.Tensor:
    """wavefunctions.py:355-371."""
    from . import graph_builders
    if isinstance(inputs, graph_builders.ConfigsVariable):
      engine = self._bind(inputs)
      return AmplitudeTensor(self, engine, None)
    arr = np.asarray(inputs, np.float32)
    if arr.ndim != 2 or (self._n_sites is not None and arr.shape[1] != self._n_sites):
      raise ValueError('Input tensor has wrong shape.')
    if self._engine is None:
      raise ValueError('apply the wavefunction to the CONFIGS variable first '
                       '(graph_builders.get_configs) so that it is bound to a GPU engine')
    return AmplitudeTensor(self, self._engine, arr)

  def _update_norm(self, batch_of_amplitudes, max_value):
    from . import parallel
    if (isinstance(batch_of_amplitudes, AmplitudeTensor) and batch_of_amplitudes.configs is None
        and batch_of_amplitudes.wavefunction is self):
      if parallel.world_size() == 1:
        self._engine.update_norm(max_value)        # max-reduce on the GPU
      else:                                        # ... and a one-float MAX all-reduce in stream
        self._engine.update_norm_dist(parallel.collective(), max_value)
      return
    log_max = self._global_log_max(batch_of_amplitudes)
    max_log = np.log(np.float32(max_value))
    if log_max is not None and log_max > max_log:
      self._set_shift(np.float32(self._get_shift() + (log_max - max_log)))

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:373-388."""
    fcnn_params = {
        'num_layers': hparams.num_fc_layers,
        'layer_size': hparams.fc_layer_size,
        'output_activation': layers.NONLINEARITIES[hparams.output_activation],
        'nonlinearity': layers.NONLINEARITIES[hparams.nonlinearity],
    }
    if name:
      fcnn_params['name'] = name
    return cls(**fcnn_params)


class RestrictedBoltzmannNetwork(FullyConnectedNetwork):
  """Extended restricted Boltzmann machine (wavefunctions.py:391-452):
  psi = exp(onsite(x) + sum_h log cosh(Linear(H)([Linear(H), nonlinearity] x num_layers (x)))_h
            - exp_norm_shift),  onsite = Linear(1).
  num_layers = 0 is the classic RBM.  Same engine, same kernels as the fully-connected ansatz
  with a log-cosh output epilogue and the rank-2 onsite update (csrc/mlp.hip, RBM variants)."""
  _ansatz = 'rbm'

  def __init__(self, num_layers: int, layer_size: int,
               nonlinearity=layers.NONLINEARITIES['relu'],
               name: str = 'restricted_boltzmann_network'):
    super(RestrictedBoltzmannNetwork, self).__init__(
        num_layers=num_layers, layer_size=layer_size, nonlinearity=nonlinearity,
        output_activation=layers.NONLINEARITIES['exp'], name=name)

  def _shapes(self):
    """Creation order of the snt.Linear variables: Sonnet v1 creates them when a module is first
    connected, and _build (wavefunctions.py:436-437) connects the onsite layer -- the LAST
    module constructed, hence `linear_{num_layers+1}` -- before the Sequential."""
    n, h, L = self._n_sites, self._layer_size, self._num_layers
    u = self._unique_name
    names = ['%s/linear_%d/w' % (u, L + 1), '%s/linear_%d/b' % (u, L + 1)]
    shapes = [(n, 1), (1,)]
    fan_in = n
    for l in range(L + 1):
      lin = 'linear' if l == 0 else 'linear_%d' % l
      names += ['%s/%s/w' % (u, lin), '%s/%s/b' % (u, lin)]
      shapes += [(fan_in, h), (h,)]
      fan_in = h
    return names, shapes

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:440-452."""
    rbm_params = {
        'num_layers': hparams.num_fc_layers,
        'layer_size': hparams.fc_layer_size,
        'nonlinearity': layers.NONLINEARITIES[hparams.nonlinearity],
    }
    if name:
      rbm_params['name'] = name
    return cls(**rbm_params)


class Conv2DNetwork(FullyConnectedNetwork):
  """[Conv2dPeriodic(num_filters, kernel_size), nonlinearity] x (num_layers - 1),
  Conv2dPeriodic, reduce_sum over sites and channels, (- exp_norm_shift), exp
  (wavefunctions.py:531-615; layers.Conv2dPeriodic, layers.py:89-160).  Inputs are reshaped to
  [-1, size_x, size_y, 1]; the kernels are the periodic implicit-GEMM family of csrc/conv.hip."""
  _ansatz = 'conv_2d'

  def __init__(self, num_layers: int, num_filters: int, kernel_size: int, size_x: int,
               size_y: int, nonlinearity=layers.NONLINEARITIES['relu'],
               output_activation=layers.NONLINEARITIES['exp'], name: str = 'conv_2d_network'):
    super(Conv2DNetwork, self).__init__(
        num_layers=num_layers, layer_size=num_filters, nonlinearity=nonlinearity,
        output_activation=output_activation, name=name)
    self._num_filters = num_filters
    self._kernel_size = kernel_size
    self._size_x = size_x
    self._size_y = size_y

  def _conv_scopes(self):
    """Variable scopes of the snt.Conv2D modules in connection order."""
    return ['conv_2d_periodic' if l == 0 else 'conv_2d_periodic_%d' % l
            for l in range(self._num_layers)]

  def _shapes(self):
    if self._n_sites != self._size_x * self._size_y:
      raise ValueError('Input tensor has wrong shape.')        # tf.reshape fails in the reference
    k, f, u = self._kernel_size, self._num_filters, self._unique_name
    names, shapes, cin = [], [], 1
    for scope in self._conv_scopes():
      names += ['%s/%s/conv_2d/w' % (u, scope), '%s/%s/conv_2d/b' % (u, scope)]
      shapes += [(k, k, cin, f), (f,)]
      cin = f
    return names, shapes

  def initialize(self, seed=None):
    """snt.Conv2D defaults: w ~ truncated normal(sigma = 1/sqrt(k*k*in_channels)), b = 0."""
    if self._n_sites is None:
      raise ValueError('wavefunction is not connected to inputs yet')
    rng = np.random.default_rng(seed)
    parts = []
    for shp in self._shapes()[1]:
      if len(shp) == 4:
        w = rng.standard_normal(shp)
        bad = np.abs(w) > 2
        while bad.any():
          w[bad] = rng.standard_normal(int(bad.sum()))
          bad = np.abs(w) > 2
        parts.append((w / np.sqrt(shp[0] * shp[1] * shp[2])).ravel())
      else:
        parts.append(np.zeros(shp).ravel())
    self._set_theta(np.concatenate(parts).astype(np.float32))

  def _engine_spec(self):
    spec = super(Conv2DNetwork, self)._engine_spec()
    spec.update(kernel_size=self._kernel_size, size_x=self._size_x, size_y=self._size_y)
    return spec

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:600-615."""
    conv_2d_params = {
        'num_layers': hparams.num_conv_layers,
        'num_filters': hparams.num_conv_filters,
        'kernel_size': hparams.kernel_size,
        'size_x': hparams.size_x,
        'size_y': hparams.size_y,
        'output_activation': layers.NONLINEARITIES[hparams.output_activation],
        'nonlinearity': layers.NONLINEARITIES[hparams.nonlinearity],
    }
    if name:
      conv_2d_params['name'] = name
    return cls(**conv_2d_params)


class ResNet2D(Conv2DNetwork):
  """Conv2dPeriodic, then num_blocks x ResBlock2d (x + conv(selu(conv(x)))), reduce_sum,
  (- exp_norm_shift), exp   (wavefunctions.py:710-809; layers.ResBlock2d, layers.py:163-229).
  The reference only has the plain block for 2D (bottleneck=True names a class layers.py does not
  define) and a block only type-checks at stride 1, so those are the supported settings."""
  _ansatz = 'res_net_2d'

  def __init__(self, num_blocks: int, num_filters: int, kernel_size: int, conv_stride: int,
               size_x: int, size_y: int, bottleneck: bool = False,
               output_activation=layers.NONLINEARITIES['exp'], name: str = 'res_net_2d'):
    if bottleneck:
      raise AttributeError("module 'layers' has no attribute 'BottleneckResBlock2d'")
    if conv_stride != 1:
      raise ValueError('Inputs shape is not compatable with filters.')   # layers.py:218-219
    super(ResNet2D, self).__init__(
        num_layers=num_blocks, num_filters=num_filters, kernel_size=kernel_size, size_x=size_x,
        size_y=size_y, nonlinearity=layers.NONLINEARITIES['relu'],
        output_activation=output_activation, name=name)
    self._num_blocks = num_blocks
    self._conv_stride = conv_stride
    self._bottleneck = bottleneck

  def _conv_scopes(self):
    scopes = ['conv_2d_periodic']
    for blk in range(self._num_blocks):
      block = 'res_block_2d' if blk == 0 else 'res_block_2d_%d' % blk
      scopes += ['%s/first_conv' % block, '%s/second_conv' % block]
    return scopes

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:794-809."""
    res_net_2d_params = {
        'num_blocks': hparams.num_resnet_blocks,
        'num_filters': hparams.num_conv_filters,
        'kernel_size': hparams.kernel_size,
        'conv_stride': hparams.conv_strides,
        'size_x': hparams.size_x,
        'size_y': hparams.size_y,
        'output_activation': layers.NONLINEARITIES[hparams.output_activation],
    }
    if name:
      res_net_2d_params['name'] = name
    return cls(**res_net_2d_params)


class Conv1DNetwork(Conv2DNetwork):
  """[Conv1dPeriodic(num_filters, kernel_size), nonlinearity] x (num_layers - 1), Conv1dPeriodic,
  reduce_sum over sites and channels, (- exp_norm_shift), exp   (wavefunctions.py:455-527;
  layers.Conv1dPeriodic, layers.py:24-86).  Inputs are expanded to [B, N, 1]; the kernels are those
  of the 2-D types on an N x 1 lattice with k x 1 taps and the 1-D padding rule (an even kernel
  pads k/2 in front and k/2 - 1 behind, layers.py:66-72 -- the mirror image of the 2-D module)."""
  _ansatz = 'conv_1d'

  def __init__(self, num_layers: int, num_filters: int, kernel_size: int,
               nonlinearity=layers.NONLINEARITIES['relu'],
               output_activation=layers.NONLINEARITIES['exp'], name: str = 'conv_1d_network'):
    super(Conv1DNetwork, self).__init__(
        num_layers=num_layers, num_filters=num_filters, kernel_size=kernel_size, size_x=0, size_y=1,
        nonlinearity=nonlinearity, output_activation=output_activation, name=name)

  def _conv_scopes(self):
    return ['conv_1d_periodic' if l == 0 else 'conv_1d_periodic_%d' % l
            for l in range(self._num_layers)]

  def _shapes(self):
    k, f, u = self._kernel_size, self._num_filters, self._unique_name
    names, shapes, cin = [], [], 1
    for scope in self._conv_scopes():
      names += ['%s/%s/conv_1d/w' % (u, scope), '%s/%s/conv_1d/b' % (u, scope)]
      shapes += [(k, cin, f), (f,)]
      cin = f
    return names, shapes

  def initialize(self, seed=None):
    """snt.Conv1D defaults: w ~ truncated normal(sigma = 1/sqrt(k*in_channels)), b = 0."""
    if self._n_sites is None:
      raise ValueError('wavefunction is not connected to inputs yet')
    rng = np.random.default_rng(seed)
    parts = []
    for shp in self._shapes()[1]:
      if len(shp) == 3:
        w = rng.standard_normal(shp)
        bad = np.abs(w) > 2
        while bad.any():
          w[bad] = rng.standard_normal(int(bad.sum()))
          bad = np.abs(w) > 2
        parts.append((w / np.sqrt(shp[0] * shp[1])).ravel())
      else:
        parts.append(np.zeros(shp).ravel())
    self._set_theta(np.concatenate(parts).astype(np.float32))

  def _engine_spec(self):
    spec = FullyConnectedNetwork._engine_spec(self)
    spec.update(kernel_size=self._kernel_size, size_x=0, size_y=0)
    return spec

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:513-527."""
    conv_1d_params = {
        'num_layers': hparams.num_conv_layers,
        'num_filters': hparams.num_conv_filters,
        'kernel_size': hparams.kernel_size,
        'output_activation': layers.NONLINEARITIES[hparams.output_activation],
        'nonlinearity': layers.NONLINEARITIES[hparams.nonlinearity],
    }
    if name:
      conv_1d_params['name'] = name
    return cls(**conv_1d_params)


class ResNet1D(Conv1DNetwork):
  """Conv1dPeriodic, then num_blocks x ResBlock1d (x + conv(selu(conv(x))), layers.py:290-293),
  reduce_sum, (- exp_norm_shift), exp   (wavefunctions.py:618-707).  Plain blocks at stride 1 are
  supported (a strided block does not type-check against its shortcut, layers.py:281-282;
  bottleneck blocks are outside the MI355X hot path)."""
  _ansatz = 'res_net_1d'

  def __init__(self, num_blocks: int, num_filters: int, kernel_size: int, conv_stride: int,
               bottleneck: bool = False, output_activation=layers.NONLINEARITIES['exp'],
               name: str = 'res_net_1d'):
    if bottleneck:
      raise NotImplementedError('BottleneckResBlock1d is outside the MI355X hot path')
    if conv_stride != 1:
      raise ValueError('Inputs shape is not compatable with filters.')
    super(ResNet1D, self).__init__(
        num_layers=num_blocks, num_filters=num_filters, kernel_size=kernel_size,
        nonlinearity=layers.NONLINEARITIES['relu'], output_activation=output_activation, name=name)
    self._num_blocks = num_blocks
    self._conv_stride = conv_stride
    self._bottleneck = bottleneck

  def _conv_scopes(self):
    scopes = ['conv_1d_periodic']
    for blk in range(self._num_blocks):
      block = 'res_block_1d' if blk == 0 else 'res_block_1d_%d' % blk
      scopes += ['%s/first_conv' % block, '%s/second_conv' % block]
    return scopes

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:692-707."""
    res_net_1d_params = {
        'num_blocks': hparams.num_resnet_blocks,
        'num_filters': hparams.num_conv_filters,
        'kernel_size': hparams.kernel_size,
        'conv_stride': hparams.conv_strides,
        'output_activation': layers.NONLINEARITIES[hparams.output_activation],
    }
    if name:
      res_net_1d_params['name'] = name
    return cls(**res_net_1d_params)


def check_adjacency(adj, num_sites=None) -> np.ndarray:
  """The adjacency list of GraphConvNetwork as an int32 [N, k] array, or ValueError: a table that
  loads 1-D (one column -- the reference fails there too), a row count other than num_sites, an
  entry outside [0, N)."""
  adj = np.asarray(adj)
  if adj.ndim != 2:
    raise ValueError('gnn: the adjacency list must be a 2-D table [num_sites, k], got shape %s'
                     % (adj.shape,))
  if adj.size and not np.issubdtype(adj.dtype, np.integer):
    raise ValueError('gnn: the adjacency list must hold integers')
  n = adj.shape[0] if num_sites is None else num_sites
  if adj.shape[0] != n:
    raise ValueError('gnn: the adjacency list has %d rows, num_sites is %d' % (adj.shape[0], n))
  if adj.size and (adj.min() < 0 or adj.max() >= n):
    raise ValueError('gnn: adjacency list entries must lie in [0, %d)' % n)
  return np.ascontiguousarray(adj, dtype=np.int32)


class GraphConvNetwork(Conv2DNetwork):
  """[GraphConvLayer(num_filters, adj), nonlinearity] x (num_layers - 1), GraphConvLayer,
  reduce_sum over sites and channels, (- exp_norm_shift), exp   (wavefunctions.py:1083-1154;
  layers.GraphConvLayer, layers.py:415-451).  A layer gathers x[:, adj] -> [B, N, k, Cin] and
  applies snt.Conv2D with a 1 x k kernel and VALID padding: a 1 x k convolution whose taps are
  read off the table.  The kernels are the general convolution path's with table-driven gathers
  (csrc/conv_general.hip)."""
  _ansatz = 'gnn'

  def __init__(self, num_layers: int, num_filters: int, adj: np.ndarray,
               nonlinearity=layers.NONLINEARITIES['relu'],
               output_activation=layers.NONLINEARITIES['exp'], name: str = 'graph_conv_network'):
    adj = check_adjacency(adj)
    super(GraphConvNetwork, self).__init__(
        num_layers=num_layers, num_filters=num_filters, kernel_size=int(adj.shape[1]), size_x=0,
        size_y=0, nonlinearity=nonlinearity, output_activation=output_activation, name=name)
    self._adj = adj

  def _conv_scopes(self):
    return ['graph_conv_layer' if l == 0 else 'graph_conv_layer_%d' % l
            for l in range(self._num_layers)]

  def _shapes(self):
    check_adjacency(self._adj, self._n_sites)           # tf.gather with a table of another graph fails
    k, f, u = self._kernel_size, self._num_filters, self._unique_name
    names, shapes, cin = [], [], 1
    for scope in self._conv_scopes():
      names += ['%s/%s/conv_2d/w' % (u, scope), '%s/%s/conv_2d/b' % (u, scope)]
      shapes += [(1, k, cin, f), (f,)]
      cin = f
    return names, shapes

  def _bind(self, configs_var):
    check_adjacency(self._adj, configs_var.shape[1])
    return super(GraphConvNetwork, self)._bind(configs_var)

  def _engine_spec(self):
    spec = FullyConnectedNetwork._engine_spec(self)
    # the graph as bytes: hashable and compared by value, so psi and its dc_ copy share one ctx and
    # two different graphs never do
    spec.update(kernel_size=self._kernel_size, size_x=0, size_y=0, adjacency=self._adj.tobytes())
    return spec

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:1138-1154; the path is read as given (relative to the working directory)."""
    adj = np.genfromtxt(hparams.adjacency_list_path, dtype=int)
    gnn_params = {
        'num_layers': hparams.num_conv_layers,
        'num_filters': hparams.num_conv_filters,
        'adj': check_adjacency(adj, hparams.num_sites),
        'output_activation': layers.NONLINEARITIES[hparams.output_activation],
        'nonlinearity': layers.NONLINEARITIES[hparams.nonlinearity],
    }
    if name:
      gnn_params['name'] = name
    return cls(**gnn_params)


class ProjectedBDG(FullyConnectedNetwork):
  """Gutzwiller-projected BCS (RVB) state (wavefunctions.py:876-928): psi(x) = det M(x), M[r][c] = F[U_r][D_c] over
  the up sites U and the down sites D of x in ascending order, F the pairing matrix (the only variable,
  projected_bdg/pairing_matrix [1, N, N]); psi = sign(det M) exp(ln|det M| - exp_norm_shift).  Signed amplitudes
  without any lattice geometry.  The kernels (csrc/pbdg.hip) keep M^-1 of every chain in LDS: determinant ratios
  and rank-2 updates per Monte Carlo move, a fresh factorisation for amplitudes and local energies."""
  _ansatz = 'pbdg'

  def __init__(self, num_sites: int, name: str = 'projected_bdg'):
    num_sites = int(num_sites)
    if num_sites < 2 or num_sites % 2:
      raise ValueError('pbdg: num_sites must be even (as many up as down spins), got %d' % num_sites)
    if num_sites > 256:
      raise NotImplementedError('pbdg: num_sites > 256 is not supported by the HIP kernels')
    super(ProjectedBDG, self).__init__(num_layers=1, layer_size=1, name=name)
    self._num_sites = num_sites

  def _shapes(self):
    if self._n_sites is not None and self._n_sites != self._num_sites:
      raise ValueError('Input tensor has wrong shape.')
    n = self._num_sites
    return ['%s/pairing_matrix' % self._unique_name], [(1, n, n)]

  def initialize(self, seed=None):
    """tf.get_variable's default glorot_uniform on [1, N, N]: fan_in = fan_out = N, U(-sqrt(3/N), sqrt(3/N))."""
    n = self._num_sites
    limit = np.sqrt(6.0 / (n + n))
    rng = np.random.default_rng(seed)
    self._set_theta(rng.uniform(-limit, limit, size=n * n).astype(np.float32))

  def _maybe_initialize(self):
    if self._n_sites is not None and self._get_theta(allow_none=True) is None:
      seed = os.environ.get('CGS_VMC_INIT_SEED')
      self.initialize(None if seed is None else int(seed) + _init_count())

  def _engine_spec(self):
    return dict(ansatz=self._ansatz, num_layers=1, layer_size=1, nonlinearity='relu', output_activation='exp')

  def _global_log_max(self, batch_of_amplitudes):
    """log(max_b psi_b) of the SIGNED amplitudes over all ranks, as the reference takes it (wavefunctions.py:250, 283):
    the largest logit among the chains with psi > 0 (a sign bit clear -- psi may underflow to +0 -- and a finite
    logit), or None where there is none (the reference writes NaN into the shift there: SURVEY.md B10)."""
    from . import parallel
    if isinstance(batch_of_amplitudes, AmplitudeTensor) and batch_of_amplitudes.wavefunction is self:
      logit, psi = self._engine.amplitude(batch_of_amplitudes.configs, self._which)
      pos = ~np.signbit(psi) & np.isfinite(logit)
      top = float(np.max(logit[pos])) if pos.any() else -np.inf
      top = np.float32(parallel.allreduce_max(top))
      if not np.isfinite(top):
        return None
      gap = np.float32(top - np.float32(self._get_shift()))
      with np.errstate(over='ignore'):
        psi_max = np.exp(gap, dtype=np.float32)
      if np.isfinite(psi_max) and psi_max > 0:
        return np.float32(np.log(psi_max))
      return gap
    psi = np.asarray(batch_of_amplitudes._run())
    top = parallel.allreduce_max(float(np.max(psi)))
    if not top > 0:
      return None
    return np.float32(np.log(np.float32(top)))

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:915-928."""
    params = {'num_sites': hparams.num_sites}
    if name:
      params['name'] = name
    return cls(**params)


class FullyConnectedNNB(FullyConnectedNetwork):
  """Neural-network backflow (wavefunctions.py:931-998): a relu trunk of num_layers snt.Linear(layer_size) layers and a
  pairing layer snt.Linear(N^2); psi(x) = det M(x), M[r][c] = F(x)[U_r][D_c] with F(x) = out.reshape(N, N) over the up
  sites U and the down sites D of x in ascending order.  Signed amplitudes and no exponent shift (the reference returns
  tf.linalg.det as it is): normalize_batch / update_norm return None.  The kernels (csrc/nnb.hip) run the trunk and the
  pairing layer on the general dense path and factorise every M in LDS; they keep (ln|det M|, sign) throughout."""
  _ansatz = 'fully_connected_nnb'
  MAX_SITES, MAX_UNITS, MAX_LAYERS = 256, 512, 16     # plan.hpp PLAN_NNB_*

  def __init__(self, num_sites: int, num_layers: int, layer_sizes, name: str = 'fully_connected_nnb'):
    num_sites, num_layers = int(num_sites), int(num_layers)
    sizes = [int(s) for s in layer_sizes]
    if num_sites < 2 or num_sites % 2:
      raise ValueError('fully_connected_nnb: num_sites must be even (as many up as down spins), got %d' % num_sites)
    if len(sizes) != num_layers:
      raise ValueError('fully_connected_nnb: layer_sizes must hold num_layers entries')
    if num_layers < 1:
      raise NotImplementedError('fully_connected_nnb: num_layers = 0 is not supported by the HIP kernels')
    if len(set(sizes)) != 1:
      raise NotImplementedError('fully_connected_nnb: hidden layers of unequal width are not supported')
    if num_sites > self.MAX_SITES or sizes[0] > self.MAX_UNITS or num_layers > self.MAX_LAYERS or sizes[0] < 1:
      raise NotImplementedError('fully_connected_nnb: the HIP kernels cover num_sites <= %d, layer size <= %d and '
                                'num_layers <= %d' % (self.MAX_SITES, self.MAX_UNITS, self.MAX_LAYERS))
    super(FullyConnectedNNB, self).__init__(num_layers=num_layers, layer_size=sizes[0], name=name)
    self._exp_norm_shift = None          # no add_exp_normalization: psi is the determinant itself
    self._num_sites = num_sites
    self._layer_sizes = sizes

  def _shapes(self):
    if self._n_sites is not None and self._n_sites != self._num_sites:
      raise ValueError('Input tensor has wrong shape.')
    n, h, u = self._num_sites, self._layer_size, self._unique_name
    names, shapes, fan_in = [], [], n
    for l in range(self._num_layers + 1):
      out = h if l < self._num_layers else n * n
      lin = 'linear' if l == 0 else 'linear_%d' % l
      names += ['%s/%s/w' % (u, lin), '%s/%s/b' % (u, lin)]
      shapes += [(fan_in, out), (out,)]
      fan_in = out
    return names, shapes

  def initialize(self, seed=None):
    if self._n_sites is None:
      self._n_sites = self._num_sites
    super(FullyConnectedNNB, self).initialize(seed)

  def _engine_spec(self):
    return dict(ansatz=self._ansatz, num_layers=self._num_layers, layer_size=self._layer_size,
                nonlinearity='relu', output_activation='exp')

  def _bind(self, configs_var):
    if configs_var.shape[1] != self._num_sites:
      raise ValueError('Input tensor has wrong shape.')
    return super(FullyConnectedNNB, self)._bind(configs_var)

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:982-998."""
    params = {'num_sites': hparams.num_sites, 'num_layers': hparams.num_fc_layers,
              'layer_sizes': [hparams.fc_layer_size] * hparams.num_fc_layers}
    if name:
      params['name'] = name
    return cls(**params)


def check_lin_tables(num_sites, top_lin_table, bot_lin_table, length):
  """The two Lin tables of FullVector as int32 arrays, or ValueError naming the offender: num_sites odd, a table that
  is not a 1-D integer array of 2^(num_sites/2) entries, an Sz = 0 configuration whose index top[t] + bot[b] leaves
  [0, length).  A configuration pairs an upper half-word of N/2 - k set bits with a lower one of k, so per popcount
  class the smallest and the largest entry decide (plan.hpp plan_edvec_check_tables)."""
  num_sites = int(num_sites)
  if num_sites < 2 or num_sites % 2:
    raise ValueError('ed_vector: num_sites must be even (the Lin tables address the Sz = 0 sector), got %d' % num_sites)
  h = num_sites // 2
  tables = []
  for label, table in (('top_lin_table', top_lin_table), ('bot_lin_table', bot_lin_table)):
    table = np.asarray(table)
    if table.ndim != 1 or table.size != 1 << h:
      raise ValueError('ed_vector: %s must be a 1-D table of 2^(num_sites/2) = %d entries, got shape %s'
                       % (label, 1 << h, table.shape))
    if not np.issubdtype(table.dtype, np.integer):
      raise ValueError('ed_vector: %s must hold integers, got %s' % (label, table.dtype))
    if table.min() < -2 ** 31 or table.max() >= 2 ** 31:
      raise ValueError('ed_vector: %s has entries beyond 32 bits' % label)
    tables.append(np.ascontiguousarray(table, dtype=np.int32))
  top, bot = tables
  halves = np.arange(1 << h)
  pop = np.zeros(1 << h, np.int64)
  for i in range(h):
    pop += (halves >> i) & 1
  for k in range(h + 1):
    t, b = top[pop == h - k].astype(np.int64), bot[pop == k].astype(np.int64)
    lo, hi = t.min() + b.min(), t.max() + b.max()
    if lo < 0 or hi >= length:
      raise ValueError('ed_vector: an Sz = 0 configuration with %d up spins in its lower half has index %d outside '
                       '[0, %d)' % (k, lo if lo < 0 else hi, length))
  return top, bot


class FullVector(FullyConnectedNetwork):
  """State vector addressed through Lin's two tables (wavefunctions.py:1001-1080): with bot = sum_{i < N/2} [s_i > 0] 2^i
  and top = sum_{i < N/2} [s_{N/2+i} > 0] 2^i, psi(x) = ed_vector[top_lin_table[top] + bot_lin_table[bot]] -- the entry
  itself, signed and possibly zero, the only variable (full_vector/ed_vector [len]).  No exponent shift:
  normalize_batch / update_norm return None.  An exact (or Lanczos) eigenstate loaded here has E_loc = E0 on every
  configuration; trained, it bounds what any ansatz can reach on the cluster.  The kernels (csrc/edvec.hip) are
  dependent gathers and a collision-safe scatter."""
  _ansatz = 'ed_vector'
  MAX_SITES = 28                      # plan.hpp PLAN_EDVEC_MAX_SITES

  def __init__(self, num_sites: int, top_lin_table, bot_lin_table, initial_vector, name: str = 'full_vector'):
    num_sites = int(num_sites)
    initial_vector = np.asarray(initial_vector)
    if initial_vector.ndim != 1 or initial_vector.size < 1:
      raise ValueError('ed_vector: the vector must be 1-D and not empty, got shape %s' % (initial_vector.shape,))
    top, bot = check_lin_tables(num_sites, top_lin_table, bot_lin_table, initial_vector.size)
    if num_sites > self.MAX_SITES:
      raise NotImplementedError('ed_vector: num_sites > %d is not supported by the HIP kernels' % self.MAX_SITES)
    super(FullVector, self).__init__(num_layers=1, layer_size=int(initial_vector.size), name=name)
    self._exp_norm_shift = None          # no add_exp_normalization: psi is the entry itself
    self._num_sites = num_sites
    self._top_lin_table, self._bot_lin_table = top, bot
    self._initial_vector = np.ascontiguousarray(initial_vector, dtype=np.float32)

  def _shapes(self):
    if self._n_sites is not None and self._n_sites != self._num_sites:
      raise ValueError('Input tensor has wrong shape.')
    return ['%s/ed_vector' % self._unique_name], [(self._initial_vector.size,)]

  def initialize(self, seed=None):
    """The variable's initializer is the vector the ansatz was built from."""
    self._set_theta(self._initial_vector.copy())

  def _maybe_initialize(self):
    if self._n_sites is not None and self._get_theta(allow_none=True) is None:
      self.initialize()

  def _engine_spec(self):
    # the tables as bytes: hashable and compared by value, so psi and its dc_ copy share one ctx
    return dict(ansatz=self._ansatz, num_layers=1, layer_size=int(self._initial_vector.size), nonlinearity='relu',
                output_activation='exp', lin_tables=self._top_lin_table.tobytes() + self._bot_lin_table.tobytes())

  def _bind(self, configs_var):
    if configs_var.shape[1] != self._num_sites:
      raise ValueError('Input tensor has wrong shape.')
    return super(FullVector, self)._bind(configs_var)

  @classmethod
  def from_hparams(cls, hparams, name: str = '') -> 'Wavefunction':
    """wavefunctions.py:1062-1080: the three files are read from hparams.checkpoint_dir."""
    path = lambda f: os.path.join(hparams.checkpoint_dir, f)
    params = {
        'num_sites': hparams.num_sites,
        'top_lin_table': np.atleast_1d(np.genfromtxt(path(hparams.top_lin_table_file), dtype=int)),
        'bot_lin_table': np.atleast_1d(np.genfromtxt(path(hparams.bot_lin_table_file), dtype=int)),
        'initial_vector': np.atleast_1d(np.genfromtxt(path(hparams.ed_vector_file), dtype=np.float32)),
    }
    if name:
      params['name'] = name
    return cls(**params)


class ProductOfWavefunctions(Wavefunction):
  """psi(x) = psi_a(x) psi_b(x) (wavefunctions.py:107-161), e.g. a positive network on a determinant state.  One engine
  serves the product: the two factors are ordinary ctxs composed by vmc_create_product (csrc/vmc_api_prod.hip), which
  owns the chains; each factor stays bound to its own ctx for its variables and its shift.  The variables are a's then
  b's, each under the factor's own scope, so a checkpoint holds exactly the two factors' variables.  Like the
  reference's, the product has no exp_norm_shift of its own: normalize_batch / update_norm return None and the factors'
  shifts stay where they are (the library works in the log domain, nothing overflows)."""
  _ansatz = 'prod'

  def __init__(self, wf_a: Wavefunction, wf_b: Wavefunction, name: str = 'product_of_wavefunctions'):
    for wf in (wf_a, wf_b):
      if not isinstance(wf, Wavefunction):
        raise NotImplementedError('a product with a scalar factor is outside the MI355X hot path')
      if isinstance(wf, ProductOfWavefunctions):
        raise NotImplementedError("prod: a product of products has no HIP kernels")
      if not isinstance(wf, FullyConnectedNetwork):
        raise NotImplementedError("prod: a factor of type %s has no HIP kernels" % type(wf).__name__)
    if wf_a is wf_b:
      raise ValueError('prod: the two factors must be two wavefunctions')
    if not name.startswith('dc_'):      # (a deep copy keeps the dc_<name> its original's __deepcopy__ chose)
      name = '_times_'.join([wf_b._unique_name, wf_a._unique_name])
    super(ProductOfWavefunctions, self).__init__(name=name)
    self._wf_a, self._wf_b = wf_a, wf_b
    self._sub_wavefunctions += [wf_a, wf_b]

  # omega = copy.deepcopy(psi): Wavefunction.__deepcopy__ rebuilds the product from deep copies of _wf_a / _wf_b

  # training.py marks a supervisor whose values arrived on the device (vmc_transfer_params): forwarded to the factors
  @property
  def _has_values(self):
    return all(wf._has_values for wf in self._sub_wavefunctions)

  @_has_values.setter
  def _has_values(self, value):
    for wf in self._sub_wavefunctions:
      wf._has_values = value

  @property
  def _theta(self):
    return None

  @_theta.setter
  def _theta(self, value):
    if value is not None:
      raise ValueError('prod: the parameters live in the factors')
    for wf in self._sub_wavefunctions:
      if wf._engine is not None:
        wf._theta = None

  def _engine_spec(self):
    freeze = lambda spec: tuple(sorted(spec.items()))
    return dict(ansatz='prod', num_layers=0, layer_size=0,
                children=(freeze(self._wf_a._engine_spec()), freeze(self._wf_b._engine_spec())))

  def _bind(self, configs_var):
    from . import parallel
    if parallel.is_distributed():
      raise NotImplementedError("wavefunction_type 'prod' runs on one rank: a product ctx has no sharded entries")
    for wf in self._sub_wavefunctions:
      if wf._engine_spec().get('output_activation') != 'exp':
        raise NotImplementedError("prod: a dense factor needs the exp output activation (%s has %r)"
                                  % (wf._unique_name, wf._engine_spec().get('output_activation')))
    engine = configs_var._get_engine(self)
    if self._engine is engine:
      return engine
    if self._engine is not None:
      raise ValueError('wavefunction %s is already bound to another CONFIGS variable' % self._unique_name)
    which = configs_var._claim_slot(self)
    self._engine, self._which = engine, which
    n_sites = configs_var.shape[1]
    for wf, child in zip(self._sub_wavefunctions, engine.children):
      if wf._engine is not None and wf._engine is not child:
        raise ValueError('wavefunction %s is already bound to another CONFIGS variable' % wf._unique_name)
      if wf._n_sites is not None and wf._n_sites != n_sites:
        raise ValueError('Input tensor has wrong shape.')
      wf._n_sites = n_sites
      wf._shapes()                     # (the factor's own shape checks)
      host_theta = wf._theta
      wf._engine, wf._which = child, which
      if host_theta is not None:
        child.set_params(host_theta, which)
        wf._theta = None
      if wf._exp_norm_shift is not None:
        child.set_shift(float(wf._exp_norm_shift), which)
    return engine

  def _build(self, inputs) -> session_lib.Tensor:
    from . import graph_builders
    if isinstance(inputs, graph_builders.ConfigsVariable):
      return AmplitudeTensor(self, self._bind(inputs), None)
    arr = np.asarray(inputs, np.float32)
    if arr.ndim != 2 or (self._wf_a._n_sites is not None and arr.shape[1] != self._wf_a._n_sites):
      raise ValueError('Input tensor has wrong shape.')
    if self._engine is None:
      raise ValueError('apply the wavefunction to the CONFIGS variable first '
                       '(graph_builders.get_configs) so that it is bound to a GPU engine')
    return AmplitudeTensor(self, self._engine, arr)

  @classmethod
  def from_hparams(cls, hparams, name: str = ''):
    raise ValueError('Hparams initialization is not supported for product.')


class SymmetrizedWavefunction(Wavefunction):
  """psi_s(x) = sum_k chi_k psi(g_k x) (extension): the base ansatz projected onto one symmetry sector, sampled from
  |psi_s|^2 and trained with its own log-derivatives.  g_k: row[i] = f_k x[perms[k][i]] (lattice.translations,
  lattice.point_group; f_k = -1 where flips[k]), chi: the real characters of the sector (one row of
  lattice.sector_characters; None: all ones).  One engine serves it: the base is an ordinary ctx of batch_size x n_ops rows
  composed by vmc_create_symmetrized (csrc/vmc_api_symz.hip), which owns the chains; the base stays bound to its own ctx
  for its variables and its shift.  The variables ARE the base's, under the base's own scope: a checkpoint of a
  symmetrized run loads into the plain base type and the other way round.  No exp_norm_shift of its own: normalize_batch
  / update_norm return None (the library folds in the log domain, nothing overflows)."""
  _ansatz = 'symmetrized'

  def __init__(self, base: Wavefunction, perms, flips=None, characters=None, name: str = 'symmetrized_wavefunction'):
    from . import lattice
    if not isinstance(base, Wavefunction):
      raise NotImplementedError('symmetrized: the base must be a wavefunction')
    if isinstance(base, (ProductOfWavefunctions, SymmetrizedWavefunction)):
      raise NotImplementedError('symmetrized: a product or a symmetrized wavefunction cannot be the base')
    if not isinstance(base, FullyConnectedNetwork) or base._ansatz not in ('fully_connected', 'rbm', 'pbdg', 'ed_vector'):
      raise NotImplementedError('symmetrized: a base of type %s has no HIP kernels (fully_connected, rbm, pbdg and '
                                'ed_vector are taken)' % type(base).__name__)
    p = np.asarray(perms)
    if p.ndim == 1 and p.size:
      p = p.reshape(1, -1)
    if p.ndim != 2:
      raise ValueError('symmetrized: perms must have shape [n_ops, n_sites]')
    self._perms, flip = lattice.check_symmetry_ops(p, flips, p.shape[1])
    if self._perms.shape[0] > 1024:
      raise ValueError('symmetrized: at most 1024 ops')
    self._flips = None if flips is None else flip
    n_ops = self._perms.shape[0]
    chi = np.ones(n_ops) if characters is None else np.asarray(characters, np.float64)
    if chi.ndim != 1 or chi.size != n_ops:
      raise ValueError('symmetrized: one character per op required ({} for {} ops)'.format(chi.size, n_ops))
    chi = lattice.check_characters(chi, n_ops)[0]
    if not chi.any():
      raise ValueError('symmetrized: every character is zero')
    self._characters = None if characters is None else chi
    self._chi = chi
    if not name.startswith('dc_'):      # (a deep copy keeps the dc_<name> its original's __deepcopy__ chose)
      name = 'symmetrized_' + base._unique_name
    super(SymmetrizedWavefunction, self).__init__(name=name)
    self._base = base
    self._sub_wavefunctions += [base]

  # omega = copy.deepcopy(psi): Wavefunction.__deepcopy__ rebuilds it from a deep copy of _base and the same ops

  @property
  def n_ops(self) -> int:
    return int(self._perms.shape[0])

  @property
  def _has_values(self):
    return self._base._has_values

  @_has_values.setter
  def _has_values(self, value):
    self._base._has_values = value

  @property
  def _theta(self):
    return None

  @_theta.setter
  def _theta(self, value):
    if value is not None:
      raise ValueError('symmetrized: the parameters live in the base')
    if self._base._engine is not None:
      self._base._theta = None

  def ops_digest(self) -> str:
    import hashlib
    h = hashlib.sha256()
    for a in self._ops_bytes():
      h.update(a)
    return h.hexdigest()

  def _ops_bytes(self):
    flips = np.zeros(self.n_ops, np.uint8) if self._flips is None else self._flips
    return (np.ascontiguousarray(self._perms, np.int32).tobytes(), np.ascontiguousarray(flips, np.uint8).tobytes(),
            np.ascontiguousarray(self._chi, np.float64).tobytes())

  def _engine_spec(self):
    freeze = lambda spec: tuple(sorted(spec.items()))
    return dict(ansatz='symmetrized', num_layers=0, layer_size=0, base=freeze(self._base._engine_spec()),
                ops=self._ops_bytes(), ops_digest=self.ops_digest())

  def _bind(self, configs_var):
    from . import parallel
    if parallel.is_distributed():
      raise NotImplementedError("a symmetrized wavefunction runs on one rank: a symmetrized ctx has no sharded entries")
    spec = self._base._engine_spec()
    if spec.get('ansatz') in ('fully_connected', 'rbm') and spec.get('output_activation') != 'exp':
      raise NotImplementedError("symmetrized: a dense base needs the exp output activation (%s has %r)"
                                % (self._base._unique_name, spec.get('output_activation')))
    n_sites = configs_var.shape[1]
    if self._perms.shape[1] != n_sites:
      raise ValueError('symmetrized: the ops permute {} sites, the configurations have {}'.format(self._perms.shape[1], n_sites))
    base = self._base
    if base._n_sites is not None and base._n_sites != n_sites:
      raise ValueError('Input tensor has wrong shape.')
    base._n_sites = n_sites
    base._shapes()                       # (the base's own shape checks, before an engine is asked for)
    if base._engine is None and base._theta is None and not base._has_values:
      base._maybe_initialize()           # (the symmetrized ctx evaluates its initial chains: it needs parameters to do so)
    engine = configs_var._get_engine(self)
    if self._engine is engine:
      return engine
    if self._engine is not None:
      raise ValueError('wavefunction %s is already bound to another CONFIGS variable' % self._unique_name)
    which = configs_var._claim_slot(self)
    self._engine, self._which = engine, which
    child = engine.children[0]
    if base._engine is not None and base._engine is not child:
      raise ValueError('wavefunction %s is already bound to another CONFIGS variable' % base._unique_name)
    host_theta = base._theta
    base._engine, base._which = child, which
    if host_theta is not None:
      child.set_params(host_theta, which)
      base._theta = None
    if base._exp_norm_shift is not None:
      child.set_shift(float(base._exp_norm_shift), which)
    return engine

  def _build(self, inputs) -> session_lib.Tensor:
    from . import graph_builders
    if isinstance(inputs, graph_builders.ConfigsVariable):
      return AmplitudeTensor(self, self._bind(inputs), None)
    arr = np.asarray(inputs, np.float32)
    if arr.ndim != 2 or arr.shape[1] != self._perms.shape[1]:
      raise ValueError('Input tensor has wrong shape.')
    if self._engine is None:
      raise ValueError('apply the wavefunction to the CONFIGS variable first '
                       '(graph_builders.get_configs) so that it is bound to a GPU engine')
    return AmplitudeTensor(self, self._engine, arr)

  @classmethod
  def from_hparams(cls, hparams, name: str = ''):
    raise ValueError('Hparams initialization is not supported for a symmetrized wavefunction.')


class AmplitudeTensor(session_lib.Tensor):
  """psi = wavefunction(inputs); evaluates to a float32 array [rows]."""

  def __init__(self, wavefunction, engine, configs):
    self.wavefunction = wavefunction
    self.engine = engine
    self.configs = configs
    super(AmplitudeTensor, self).__init__(self._value, 'psi')

  def _value(self):
    return self.engine.amplitude(self.configs, self.wavefunction._which)[1]

  def logits(self):
    return self.engine.amplitude(self.configs, self.wavefunction._which)[0]


class _OutOfScope(Wavefunction):
  """Registered ansatz names whose kernels are not part of the MI355X hot path."""
  _kind = ''

  @classmethod
  def from_hparams(cls, hparams, name: str = ''):
    raise NotImplementedError(
        "wavefunction_type '%s' is outside the MI355X hot path (SURVEY.md 2); only "
        "'fully_connected', 'rbm', 'conv_1d', 'conv_2d', 'res_net_1d', 'res_net_2d', 'gnn', 'pbdg', 'fully_connected_nnb' and 'ed_vector' have "
        "HIP kernels" % cls._kind)


def _stub(kind):
  return type('OutOfScope_' + kind, (_OutOfScope,), {'_kind': kind})


def build_wavefunction(hparams) -> Wavefunction:
  """wavefunctions.py:1157-1196."""
  wavefunction_type = hparams.wavefunction_type
  if wavefunction_type in WAVEFUNCTION_TYPES:
    return WAVEFUNCTION_TYPES[wavefunction_type].from_hparams(hparams)
  if wavefunction_type == 'prod':
    # wavefunctions.py:1178-1194: the two factors from copies of the hparams with their own type and output activation
    children = []
    for wf_type, activation in zip(hparams.composite_wavefunction_types, hparams.composite_output_activations):
      if wf_type not in WAVEFUNCTION_TYPES:
        raise ValueError('Provided wavefunction_type is not registered.')
      child_hparams = copy.copy(hparams)
      child_hparams.set_hparam('wavefunction_type', wf_type)
      child_hparams.set_hparam('output_activation', activation)
      children.append(WAVEFUNCTION_TYPES[wf_type].from_hparams(child_hparams))
    if len(children) != 2:
      raise ValueError("wavefunction_type 'prod' needs two composite_wavefunction_types")
    return children[0] * children[1]
  if hparams.wavefunction_type in ('sum', 'diff', 'prod'):
    raise NotImplementedError('composite wavefunctions are outside the MI355X hot path')
  raise ValueError('Provided wavefunction_type is not registered.')


WAVEFUNCTION_TYPES = {
    'fully_connected': FullyConnectedNetwork,
    'rbm': RestrictedBoltzmannNetwork,
    'conv_1d': Conv1DNetwork,
    'conv_2d': Conv2DNetwork,
    'mps': _stub('mps'),
    'pbdg': ProjectedBDG,
    'fully_connected_nnb': FullyConnectedNNB,
    'res_net_1d': ResNet1D,
    'res_net_2d': ResNet2D,
    'ed_vector': FullVector,
    'gnn': GraphConvNetwork,
}

"""What the two device task layers that run the host ports' own task code share (suite/device_env.py: the ports on torch
tensors, `TArr`; suite/fused_env.py: the ports traced into an expression DAG, `SArr`).

  TaskArray        the numpy-facing array class: operators, reductions, numpy's two dispatch protocols
  make_view_class  the domain's `Physics` subclass whose `data` / `named.data` are served as TaskArrays
  episode_attrs    what a task hung on the physics at episode start
  TaskEnv          the environment skeleton: the host environment, the fields bound to tensors
  capture_step     a control step recorded into a HIP graph

numpy only at module level: suite/common.py imports this module, and the task ports import without torch.
"""
import collections

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# the numpy surface of the task ports
# ---------------------------------------------------------------------------------------------------------------------
# What `get_observation / get_reward / termination_mask` of a suite port (and the helpers of suite/common.py,
# utils/rewards.py) may call on the arrays the physics hands them: both backends serve exactly these, and each one's
# 45-task sweep (tests/test_device_env.py, tests/test_fused_env.py) only proves the calls its ports make today.
PORT_FUNCTIONS = (
    np.concatenate, np.stack, np.where, np.linalg.norm, np.einsum, np.dot, np.clip, np.cross,
    np.sum, np.mean, np.prod, np.min, np.max, np.amin, np.amax, np.all, np.any,
    np.shape, np.ndim, np.size, np.reshape, np.ravel, np.squeeze, np.expand_dims, np.broadcast_to, np.zeros_like,
    np.ones_like, np.copy, np.atleast_1d, np.transpose)
PORT_UFUNCS = (
    'add', 'subtract', 'multiply', 'true_divide', 'divide', 'power', 'negative', 'absolute', 'fabs', 'sqrt', 'square',
    'reciprocal', 'exp', 'expm1', 'log', 'log1p', 'log2', 'log10', 'sin', 'cos', 'tan', 'arcsin', 'arccos', 'arctan',
    'arctan2', 'hypot', 'sinh', 'cosh', 'tanh', 'arcsinh', 'arccosh', 'arctanh', 'maximum', 'minimum', 'sign', 'floor',
    'ceil', 'less', 'less_equal', 'greater', 'greater_equal', 'equal', 'not_equal', 'logical_and', 'logical_or',
    'logical_not', 'isfinite', 'isnan')
PORT_METHODS = ('reshape', 'ravel', 'copy', 'astype', 'squeeze', 'dot', 'clip', 'sum', 'mean', 'prod', 'min', 'max',
                'all', 'any')
# THE GAP: served by one backend only, so a port that uses one of these passes that backend's sweep and breaks the other
ONE_BACKEND_ONLY = {'SArr': (np.hstack, np.isscalar, 'flatten'), 'TArr': ()}

# operator dunder -> (op key, operands reversed); the keys are Graph.binary's op names
_BINARY_OPERATORS = {
    '__add__': ('add', False), '__radd__': ('add', True), '__sub__': ('sub', False), '__rsub__': ('sub', True),
    '__mul__': ('mul', False), '__rmul__': ('mul', True), '__truediv__': ('div', False), '__rtruediv__': ('div', True),
    '__pow__': ('pow', False), '__rpow__': ('pow', True), '__lt__': ('lt', False), '__le__': ('le', False),
    '__gt__': ('gt', False), '__ge__': ('ge', False), '__eq__': ('eq', False), '__ne__': ('ne', False),
    '__and__': ('and', False), '__rand__': ('and', True), '__or__': ('or', False), '__ror__': ('or', True)}
_UNARY_OPERATORS = {'__invert__': 'not', '__neg__': 'neg', '__abs__': 'abs'}


class TaskArray:
  """Base of the arrays the task ports compute with.  A backend supplies `_bin(key, other, reverse)` / `_un(key)` for the
  operators, `_reduce(key, x, axis, keepdims)` (key: the numpy method's name), `_clip(x, lo, hi)`, `_dot(a, b)`,
  `_reshape(shape)`, `_ufunc(name, inputs)` and its `_FUNCS` table (`shared_functions` plus its own entries)."""

  __hash__ = None

  def __pos__(self):
    return self

  def reshape(self, *shape):
    if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
      shape = tuple(shape[0])
    return self._reshape(tuple(int(s) for s in shape))

  def ravel(self): return self._reshape((-1,))
  def dot(self, other): return self._dot(self, other)
  def clip(self, lo=None, hi=None): return self._clip(self, lo, hi)
  def sum(self, axis=None, keepdims=False): return self._reduce('sum', self, axis, keepdims)
  def mean(self, axis=None, keepdims=False): return self._reduce('mean', self, axis, keepdims)
  def prod(self, axis=None, keepdims=False): return self._reduce('prod', self, axis, keepdims)
  def min(self, axis=None, keepdims=False): return self._reduce('min', self, axis, keepdims)
  def max(self, axis=None, keepdims=False): return self._reduce('max', self, axis, keepdims)
  def all(self, axis=None, keepdims=False): return self._reduce('all', self, axis, keepdims)
  def any(self, axis=None, keepdims=False): return self._reduce('any', self, axis, keepdims)

  def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
    if method != '__call__' or kwargs.get('out') is not None:
      return NotImplemented
    return self._ufunc(ufunc.__name__, inputs)

  def __array_function__(self, func, types, args, kwargs):
    fn = self._FUNCS.get(func)
    if fn is None:
      return NotImplemented
    return fn(*args, **kwargs)


def _install_operators():      # plain functions on the class: an operator costs one call more than its backend's _bin
  def binary(key, reverse):
    return lambda self, other: self._bin(key, other, reverse)

  def unary(key):
    return lambda self: self._un(key)
  for name, (key, reverse) in _BINARY_OPERATORS.items():
    setattr(TaskArray, name, binary(key, reverse))
  for name, key in _UNARY_OPERATORS.items():
    setattr(TaskArray, name, unary(key))


_install_operators()


def shared_functions(cls):
  """The `__array_function__` entries that only delegate to the array's own methods and backend hooks."""
  def reduction(key):
    return lambda x, axis=None, keepdims=False, **k: cls._reduce(key, x, axis, keepdims)
  return {
      np.sum: reduction('sum'), np.mean: reduction('mean'), np.prod: reduction('prod'), np.min: reduction('min'),
      np.max: reduction('max'), np.amin: reduction('min'), np.amax: reduction('max'), np.all: reduction('all'),
      np.any: reduction('any'), np.clip: cls._clip, np.dot: cls._dot,
      np.shape: lambda x: x.shape, np.ndim: lambda x: x.ndim, np.size: lambda x: x.size,
      np.reshape: lambda x, shape, **k: x.reshape(shape), np.ravel: lambda x, **k: x.ravel(),
      np.squeeze: lambda x, axis=None: x.squeeze(axis), np.copy: lambda x, **k: x.copy(),
      np.atleast_1d: lambda x: x if x.ndim else x.reshape(1)}


# ---------------------------------------------------------------------------------------------------------------------
# the view: the domain's Physics subclass over TaskArrays
# ---------------------------------------------------------------------------------------------------------------------
_SCALAR_FIELDS = ('time', 'ncon', 'nefc', 'solver_iter')
INT_FIELDS = ('ncon', 'nefc', 'solver_iter', 'env_mode')


def make_view_class(cls, prefix, leaf, built_by, read_only, no_step, host_attr=None):
  """`cls` (a suite domain's Physics) with `data` / `named.data` served as TaskArrays: class `prefix + cls.__name__`.
  An instance is made with `object.__new__` and needs `_host` (the host physics), `_fields` (name -> what `leaf` wants),
  `model`, `batch_size` in its `__dict__`; `build_named` adds `data` and `named`.

  leaf(view, name, entry) -> the field as a flat TaskArray, batch axes + (rows,)
  host_attr(view, name, value) -> what the view serves for an attribute of the host physics (default: the value)
  built_by / read_only / no_step: the error texts."""
  from dm_control_amd import physics as facade

  class Data:

    def __init__(self, view):
      object.__setattr__(self, '_v', view)

    def __getattr__(self, name):
      v = self._v
      entry = v._fields.get(name)
      if entry is None:
        raise AttributeError('data.%s is not served on the device (bound fields: %s)' % (name, sorted(v._fields)))
      a = leaf(v, name, entry)
      ncol = facade._FIELD_AXES.get(name, (None, None))[1]      # pylint: disable=protected-access
      if name in _SCALAR_FIELDS:
        return a[..., 0]
      if ncol:
        return a._reshape(a.shape[:-1] + (a.shape[-1] // ncol, ncol))
      return a

    def __setattr__(self, name, value):
      raise AttributeError(read_only)

  class View(cls):
    __doc__ = '`%s` with `data` / `named.data` served as task arrays (suite/task_arrays.py).' % cls.__name__
    _Data = Data

    def __init__(self):      # pylint: disable=super-init-not-called
      raise TypeError('built by ' + built_by)

    def __getattr__(self, name):
      # whatever the task hung on the physics at episode start (targets ...) and the view does not hold itself
      if name.startswith('_'):
        raise AttributeError(name)
      host = self.__dict__['_host']
      if name in host.__dict__ or hasattr(type(host), name):
        val = getattr(host, name)
        return val if host_attr is None else host_attr(self, name, val)
      raise AttributeError(name)

    # engine.py:589-622 accessors: copies in the reference, fresh arrays here
    def control(self): return self.data.ctrl.copy()
    def position(self): return self.data.qpos.copy()
    def velocity(self): return self.data.qvel.copy()
    def activation(self): return self.data.act.copy()
    def state(self): return self.get_state()
    def time(self): return self.data.time
    def timestep(self): return self.model.opt.timestep

    def get_state(self, sig=None):
      if sig is not None:
        raise NotImplementedError('state signatures are served by the facade')
      parts = [self.data.qpos, self.data.qvel] + ([self.data.act] if self.model.na else [])
      return np.concatenate(parts, axis=-1)

    def step(self, *a, **k): raise TypeError(no_step)
    forward = reset = after_reset = set_control = step

    def free(self):
      pass

    def __del__(self):
      pass
  View.__name__ = prefix + cls.__name__
  return View


def build_named(view, host_physics, fields, batched):
  """Gives `view` its `data` proxy and the `named.model` / `named.data` indexers of the facade over the view's own
  `data`, for the fields in `fields`."""
  from dm_control_amd import physics as facade
  view.__dict__['data'] = view._Data(view)
  named = facade._Named()      # pylint: disable=protected-access
  named.model = host_physics.named.model
  named.data = facade._Named()      # pylint: disable=protected-access
  axes = facade._make_axes(host_physics.model)      # pylint: disable=protected-access
  for field, (rowkind, ncol) in facade._FIELD_AXES.items():      # pylint: disable=protected-access
    if field in fields:
      cols = facade._Axis(facade._COLS[ncol]) if ncol else None      # pylint: disable=protected-access
      setattr(named.data, field, facade.FieldIndexer(lambda f=field: getattr(view.data, f), axes[rowkind], cols, batched))
  view.__dict__['named'] = named


# ---------------------------------------------------------------------------------------------------------------------
# what the task hung on the physics at episode start
# ---------------------------------------------------------------------------------------------------------------------
_NOT_ATTRS = ('model', 'batch', 'data', 'named', 'batch_size', 'legacy_step')


def task_attrs(p):
  """(name, value) of what the task set on the physics `p` (targets, radii, flags ...)."""
  return [(k, val) for k, val in vars(p).items() if not k.startswith('_') and k not in _NOT_ATTRS]


def is_episode_array(val, B):
  """Per-episode data of the environments: a float array with a leading batch axis -- any float array when B == 1, where
  the ports drop that axis (`xy[0] if B == 1 else xy`).  A device layer must keep it in memory that a restart rewrites in
  place: as a host value it would be baked into the captured graph / the generated kernel at its first value."""
  return isinstance(val, np.ndarray) and val.ndim >= 1 and val.dtype.kind == 'f' and (val.shape[0] == B or B == 1)


def episode_attrs(p, B):
  """The per-episode arrays among `task_attrs(p)`: name -> ((B, w) float array, the shape one environment's code sees)."""
  out = collections.OrderedDict()
  for k, val in task_attrs(p):
    if is_episode_array(val, B):
      batched = val.shape[0] == B and B > 1
      v = val.reshape(B, -1) if batched else val.reshape(1, -1)
      out[k] = (np.ascontiguousarray(v), tuple(val.shape[1:]) if batched else tuple(val.shape))
  return out


# ---------------------------------------------------------------------------------------------------------------------
# the environment skeleton
# ---------------------------------------------------------------------------------------------------------------------
def served_fields():
  """The fields the facade serves from the device (the rest of its named fields are derived on the host)."""
  from dm_control_amd import physics as facade
  return [n for n in facade._FIELD_AXES if n not in ('xanchor', 'xaxis', 'ten_length', 'ten_velocity')] + ['time', 'ncon']      # pylint: disable=protected-access


def field_rows(p, names, empty=False):
  """name -> rows of the batch's field, for the names the batch of `p` has (empty: also those with no rows)."""
  rows = {}
  for name in names:
    try:
      r = p.batch._rows      # pylint: disable=protected-access
      nrow = r(name)[0] if callable(r) else (r[name] if name in r else int(np.asarray(p.batch.get(name)).shape[1]))
    except Exception:      # pylint: disable=broad-except
      continue
    if nrow or empty:
      rows[name] = int(nrow)
  return rows


class TaskEnv:
  """What GenericDeviceEnv and FusedDeviceEnv share: the host environment whose task code they run, and its batch's
  fields bound to torch tensors."""

  def _load_host(self, domain, task, batch_size, precision, device_id, seed, task_kwargs, device='cuda', **physics_kwargs):
    """`suite.load` with the seed as the task's default `random`; sets torch, B, device, dtype, host_env, host_physics,
    task, model, n_sub_steps.  Returns the step limit as control.Environment counts it (float, inf: none)."""
    import torch
    from dm_control_amd import suite
    self.torch = torch
    self.B = int(batch_size)
    self.device = torch.device(device, device_id) if device == 'cuda' else torch.device('cpu')
    self.dtype = torch.float32 if precision == 32 else torch.float64
    kw = dict(task_kwargs or {})
    kw.setdefault('random', seed)
    self.host_env = suite.load(domain, task, task_kwargs=kw,
                               physics_kwargs=dict(batch_size=self.B, precision=precision, device_id=device_id, **physics_kwargs))
    p = self.host_env.physics
    self.host_physics, self.task, self.model = p, self.host_env.task, p.model
    self.n_sub_steps = int(self.host_env._n_sub_steps)      # pylint: disable=protected-access
    return self.host_env._step_limit      # pylint: disable=protected-access

  def _bind_fields(self, names, mirror=False):
    """Binds the batch's fields `names` to torch tensors (rows, B) of their own (zero copy), `self._tensors`.  mirror: the
    tensors start with the batch's current values and fields without rows are kept, empty; on a CPU device (the test
    harness: nothing to bind) they are copies."""
    torch, p = self.torch, self.host_physics
    self._tensors = {}
    for name, nrow in field_rows(p, names, empty=mirror).items():
      dt = torch.float64 if name == 'time' else torch.int32 if name in INT_FIELDS else self.dtype
      t = torch.zeros((max(nrow, 1), self.B), dtype=dt, device=self.device)
      if nrow:
        if mirror:
          t.copy_(torch.as_tensor(np.ascontiguousarray(np.asarray(p.batch.get(name)).T), device=self.device).to(dt))
        if self.device.type == 'cuda':
          p.batch.bind(name, t.data_ptr())
      self._tensors[name] = t if nrow else t[:0]

  def _stream(self):
    return self.torch.cuda.current_stream().cuda_stream if self.device.type == 'cuda' else None

  def warnings(self):
    return self.host_physics.batch.get('warning')

  def close(self):
    self._graph = None
    self.host_physics.free()


def capture_step(torch, run, carried):
  """Records `run()` (device operations only, every call the same) into a HIP graph; returns (graph, what run returned
  inside the capture: the tensors every replay rewrites).  The tensors of `carried` -- what a step reads and writes --
  are the same afterwards as before: the caller's first replay is its step."""
  saved = [t.clone() for t in carried]
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):      # warm-up off the default stream, as graph capture requires
    run()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = run()
  for t, v in zip(carried, saved):      # the warm-up run is taken back
    t.copy_(v)
  return graph, out

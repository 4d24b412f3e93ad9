"""BatchDynamics: the joint-space inertia, its products and solves, the bias forces and inverse dynamics for a whole batch,
each computed on the device by one HIP launch.

The reference asks one environment per call on the host (`mujoco.mj_fullM`, `mj_mulM`, `mj_solveM`, `mj_rne`, or reads
`mjData.qM` / `qfrc_bias` after a forward pass).  This module gives a batch the same numbers as tensors that never leave
the GPU -- what a model-based controller multiplies `jacobian.BatchJacobian`'s J, J qvel and J'f by:

  * mass_matrix():  M (B, nv, nv), dense and symmetric: mj_crb + mj_fullM, `dof_armature` on the diagonal.
  * bias():         (B, nv) = mj_rne(flg_acc=0) = mjData.qfrc_bias: Coriolis, centrifugal and gravity forces.
  * inverse(qacc):  (B, nv) = mj_rne(flg_acc=1) = M qacc + bias.
  * mul(v):         M v (mj_mulM); v (B, nv) -> (B, nv) or (B, K, nv) -> (B, K, nv).
  * solve(f):       M^-1 f (mj_solveM), the same shapes; the K right-hand sides share one factorisation.

Gravity compensation is `bias()` at qvel = 0, computed torque `inverse(qacc_desired)`, the operational-space inertia
`(J solve(J'))^-1`.

Scope: the rigid-body terms only.  `inverse()` is mj_rne, NOT mj_inverse: passive forces (springs, dampers, fluid),
actuator forces and constraint forces are not part of any result here.

Everything is computed from the qpos / qvel in device memory (csrc/dyn_core.h: kinematics of the whole tree, composite
inertias, recursive Newton-Euler, dense Cholesky), so the unit needs no output mask and can never read stale poses.  The
model constants -- the body and joint tables, `dof_armature`, `opt.gravity` and the gravity disable flag -- are read from
the compiled model when the object is made: model edits made afterwards need a new object.  A body that carries a joint
and descends from a mocap body is refused: its pose is not a function of qpos.  Mocap bodies themselves carry no dof and
are skipped.
"""
import ctypes

import numpy as np

from dm_control_amd import _native
from dm_control_amd import _unit
from dm_control_amd import mjcf_compiler

MAX_DOFS = 64
LANES = (16, 32, 64)
CHUNK = 8                      # right-hand sides per pass through the workspace (csrc/dyn_core.h kDynChunk)
LDS_TIERS = (16384, 32768, 65536)
_JNT_NV = (6, 3, 1, 1)
_INT_TABLES = ('body_parent', 'body_jntadr', 'body_jntnum', 'body_root', 'body_lastdof', 'sub_adr', 'level_adr', 'level_body',
               'jnt_type', 'jnt_qadr', 'jnt_dadr', 'dof_body', 'dof_parent', 'dof_pred', 'dof_rot', 'sub_body')
_REAL_TABLES = ('body_pos', 'body_quat', 'body_ipos', 'body_iquat', 'body_mass', 'body_inertia', 'jnt_axis', 'jnt_pos', 'jnt_qpos0',
                'dof_armature', 'gravity')


class _Tables(ctypes.Structure):      # dmc_dyn_tables
  _fields_ = [(n, ctypes.c_int32) for n in ('nb', 'nj', 'nv', 'nq', 'nlevel', 'nsub', 'nints', 'nreals')] + \
             [('ints', ctypes.c_void_p), ('reals', ctypes.c_void_p)]


def model_tables(model):
  """dict(dims, ints, reals, bodies, + every table by name) of a compiled model as dmc_dyn_create takes them
  (include/dmc_dyn.h).  Only the bodies that matter are kept, renumbered: the world, every body with a dof on its path and
  every body with a joint somewhere below it (`bodies`: their ids in the model).  Mocap bodies and whatever is welded to
  them or to the world without a joint below carry no dof and are left out."""
  m = model
  nb, nv = int(m.nbody), int(m.nv)
  if nv == 0:
    raise ValueError('dynamics: the model has no degree of freedom (nv = 0)')
  if nv > MAX_DOFS:
    raise ValueError('dynamics: nv = %d, at most %d are supported' % (nv, MAX_DOFS))
  parent = [int(p) for p in m.body_parentid]
  jntnum = [int(n) for n in m.body_jntnum]
  mocap = np.asarray(getattr(m, 'body_mocapid', np.full(nb, -1)))
  names = m.names.get('body', [None] * nb) if hasattr(m, 'names') else [None] * nb
  below_mocap = [False] * nb
  on_path = [False] * nb      # a dof on the path from the world to the body
  for b in range(1, nb):
    below_mocap[b] = below_mocap[parent[b]] or int(mocap[b]) >= 0
    on_path[b] = on_path[parent[b]] or jntnum[b] > 0
    if below_mocap[b] and jntnum[b] > 0:
      raise ValueError('dynamics: body %r carries a joint and hangs off a mocap body: its pose is not a function of qpos'
                       % (names[b] if names[b] is not None else b,))
  keep = list(on_path)
  for b in range(nb - 1, 0, -1):      # ... or a joint somewhere below (its frame is on a jointed body's path)
    if keep[b]:
      keep[parent[b]] = True
  keep[0] = True
  bodies = [b for b in range(nb) if keep[b]]
  local = {b: k for k, b in enumerate(bodies)}
  n = len(bodies)
  t = {k: [] for k in _INT_TABLES + _REAL_TABLES}
  depth = [0] * n
  lastdof = [-1] * nb
  for k, b in enumerate(bodies):
    p = parent[b] if b else 0
    t['body_parent'].append(local[p])
    depth[k] = depth[local[p]] + 1 if b else 0
    t['body_jntadr'].append(int(m.body_jntadr[b]) if jntnum[b] else 0)
    t['body_jntnum'].append(jntnum[b])
    t['body_root'].append(local[int(m.body_rootid[b])] if b else 0)
    lastdof[b] = lastdof[p] if b else -1
    for j in range(int(m.body_jntadr[b]), int(m.body_jntadr[b]) + jntnum[b]):
      lastdof[b] = int(m.jnt_dofadr[j]) + _JNT_NV[int(m.jnt_type[j])] - 1
    t['body_lastdof'].append(lastdof[b])
  subs = [[] for _ in range(n)]
  for k in range(n):
    a = k
    while True:
      subs[a].append(k)
      if a == 0:
        break
      a = t['body_parent'][a]
  t['sub_adr'] = np.concatenate([[0], np.cumsum([len(s) for s in subs])]).tolist()
  t['sub_body'] = [c for s in subs for c in s]
  nlevel = max(depth)
  order = sorted(range(1, n), key=lambda k: (depth[k], k))
  t['level_body'] = order
  t['level_adr'] = [sum(1 for k in order if depth[k] <= l) for l in range(nlevel + 1)]
  t['jnt_type'] = [int(x) for x in m.jnt_type]
  t['jnt_qadr'] = [int(x) for x in m.jnt_qposadr]
  t['jnt_dadr'] = [int(x) for x in m.jnt_dofadr]
  dof_parent = [int(x) for x in m.dof_parentid]
  pred, rot = [0] * nv, [0] * nv
  for j in range(int(m.njnt)):
    ty, d = int(m.jnt_type[j]), int(m.jnt_dofadr[j])
    before = dof_parent[d]
    if ty == 0:
      for i in range(3):
        pred[d + i], rot[d + i] = before, 0
        pred[d + 3 + i], rot[d + 3 + i] = d + 2, 1
    elif ty == 1:
      for i in range(3):
        pred[d + i], rot[d + i] = before, 1
    else:
      pred[d], rot[d] = before, int(ty == 3)
  t['dof_body'] = [local[int(b)] for b in m.dof_bodyid]
  t['dof_parent'], t['dof_pred'], t['dof_rot'] = dof_parent, pred, rot
  f64 = lambda a: np.asarray(a, dtype=np.float64)
  for name in ('body_pos', 'body_quat', 'body_ipos', 'body_iquat', 'body_mass', 'body_inertia'):
    t[name] = f64(getattr(m, name))[bodies]
  t['jnt_axis'], t['jnt_pos'] = f64(m.jnt_axis), f64(m.jnt_pos)
  t['jnt_qpos0'] = f64(m.qpos0)[np.asarray(t['jnt_qadr'], dtype=np.int64)] if m.njnt else np.zeros(0)
  t['dof_armature'] = f64(m.dof_armature)
  off = int(m.opt.disableflags) & mjcf_compiler.C['DMC_DSBL_GRAVITY']
  t['gravity'] = np.zeros(3) if off else f64(m.opt.gravity)
  out = {k: np.ascontiguousarray(t[k], dtype=np.int32).reshape(-1) for k in _INT_TABLES}
  out.update({k: np.ascontiguousarray(f64(t[k]).reshape(-1)) for k in _REAL_TABLES})
  out['ints'] = np.ascontiguousarray(np.concatenate([out[k] for k in _INT_TABLES]).astype(np.int32))
  out['reals'] = np.ascontiguousarray(np.concatenate([out[k] for k in _REAL_TABLES]))
  out['dims'] = dict(nb=n, nj=int(m.njnt), nv=nv, nq=int(m.nq), nlevel=nlevel, nsub=len(t['sub_body']))
  out['bodies'] = bodies
  return out


def workspace_reals(nb, nv, kind):
  """Reals of one environment's workspace (csrc/dyn_core.h dyn_layout): kind 0 mass_matrix / mul / solve, kind 1 bias /
  inverse."""
  o = 17 * nb + 6 * nv
  o += (10 * nb + nv * nv + nv + 2 * CHUNK * nv) if kind == 0 else (9 * nv + 18 * nb)
  return (o + 1) & ~1


def choose_lanes(nb, nv, precision, lanes_per_env=0):
  """The lanes of a wavefront that work on one environment: `lanes_per_env`, or (0) the narrowest of 16 / 32 / 64 that is
  no narrower than the model's dofs and moving bodies (64 beyond that) and whose 64 / lanes workspaces fit 64 KB of LDS."""
  if isinstance(lanes_per_env, bool) or not isinstance(lanes_per_env, (int, np.integer)) or int(lanes_per_env) not in (0,) + LANES:
    raise ValueError('lanes_per_env: expected 0 (choose), 16, 32 or 64, got %r' % (lanes_per_env,))
  rb = 8 if int(precision) == 64 else 4
  fits = lambda w: max(workspace_reals(nb, nv, 0), workspace_reals(nb, nv, 1)) * rb * (64 // w) <= LDS_TIERS[-1]
  if int(lanes_per_env):
    if not fits(int(lanes_per_env)):
      raise ValueError('lanes_per_env = %d is too small for the model: %d environments of nv = %d, %d bodies do not fit one '
                       "workgroup's LDS" % (lanes_per_env, 64 // int(lanes_per_env), nv, nb))
    return int(lanes_per_env)
  for w in LANES:
    if w >= min(64, max(nv, nb - 1)) and fits(w):
      return w
  raise ValueError('dynamics: nv = %d with %d bodies does not fit one workgroup\'s LDS' % (nv, nb))


class BatchDynamics(_unit.BatchUnit):
  """M, M v, M^-1 f, the bias forces and inverse dynamics for every environment of a batch; see the module docstring.

  physics_or_batch: a `BatchedPhysics`, or anything holding one as `.batch` (Physics) or `.physics`.
  lanes_per_env: 0 (chosen from nv and the number of bodies), 16, 32 or 64 lanes of a wavefront per environment.  fp64
  results do not depend on it.  The model's tables are read here; model edits made afterwards need a new object.
  """
  _DESTROY = 'dmc_dyn_destroy'
  _OUT_ERROR = 'out: expected a contiguous %s tensor of shape %s on %s'

  def __init__(self, physics_or_batch, lanes_per_env=0):
    batch = _unit.find_batch(physics_or_batch)
    if batch is None:
      raise TypeError('BatchDynamics needs a BatchedPhysics (or an object holding one as .batch / .physics / .host_physics)')
    self.batch, self.model = batch, batch.model
    self.tables = model_tables(self.model)
    d = self.tables['dims']
    self.nv = d['nv']
    self.lanes_per_env = choose_lanes(d['nb'], d['nv'], batch.precision, lanes_per_env)
    self.output_mask = 0      # nothing a step launch writes is read: everything is computed from qpos / qvel
    tb = _Tables(d['nb'], d['nj'], d['nv'], d['nq'], d['nlevel'], d['nsub'], self.tables['ints'].size, self.tables['reals'].size,
                 self.tables['ints'].ctypes.data, self.tables['reals'].ctypes.data)
    self._ptr = ctypes.c_void_p()
    _native.check(_native.lib().dmc_dyn_create(batch._ptr, ctypes.byref(tb), self.lanes_per_env, ctypes.byref(self._ptr)))
    self._keep = None

  def info(self):
    a = np.zeros(10, dtype=np.int32)
    _native.check(_native.lib().dmc_dyn_info(self._ptr, a.ctypes.data))
    return dict(zip(('B', 'precision', 'nv', 'nbody', 'lanes_per_env', 'envs_per_block', 'lds_bytes', 'rne_lds_bytes', 'chunk',
                     'levels'), (int(x) for x in a)))

  def _input(self, x, shapes, what):
    """`x` as a contiguous tensor in the batch precision on the batch's device; its shape must be one of `shapes`."""
    torch, dev, dt = self._torch()
    if isinstance(x, torch.Tensor):
      if x.dtype != dt:
        raise ValueError('%s: expected dtype %s, got %s' % (what, dt, x.dtype))
      if x.device != dev:
        raise ValueError('%s: expected a tensor on %s, got %s' % (what, dev, x.device))
      shape = tuple(x.shape)
    else:
      a = np.asarray(x)
      if a.dtype.kind not in 'fiu':
        raise ValueError('%s: expected real numbers, got dtype %s' % (what, a.dtype))
      shape = a.shape
    if not any(len(shape) == len(s) and all(w is None or w == v for w, v in zip(s, shape)) for s in shapes):
      raise ValueError('%s: expected shape %s, got %s' % (what, ' or '.join(str(s).replace('None', 'K') for s in shapes), shape))
    if len(shape) == 3 and shape[1] < 1:
      raise ValueError('%s: K = %d, at least one vector per environment is needed' % (what, shape[1]))
    return (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=dt, device=dev)).contiguous()

  def mass_matrix(self, out=None, stream=None):
    """M(q) of every environment in one launch: (B, nv, nv) in the batch precision, dense, exactly symmetric, exact zeros
    where neither dof is an ancestor of the other; `dof_armature` on the diagonal (mj_crb + mj_fullM).  Asynchronous on
    `stream` (a torch stream or a raw handle; default: torch's current stream), capturable in a HIP graph; `out` is written
    in place.  Every element is written.  The host is never read."""
    _, _, dt = self._torch()
    B, nv = self.batch.batch_size, self.nv
    res = self._tensor((B, nv, nv), dt, out)
    _native.check(_native.lib().dmc_dyn_mass_matrix(self._ptr, res.data_ptr(), self.stream_handle(stream)))
    return res

  def bias(self, out=None, stream=None):
    """(B, nv) = mj_rne(flg_acc=0) = mjData.qfrc_bias at the qpos / qvel in device memory: Coriolis, centrifugal and
    gravity forces (no gravity where the model disables it).  Passive, actuator and constraint forces are NOT included.
    One launch; `out` and `stream` as in `mass_matrix`."""
    _, _, dt = self._torch()
    res = self._tensor((self.batch.batch_size, self.nv), dt, out)
    _native.check(_native.lib().dmc_dyn_bias(self._ptr, res.data_ptr(), self.stream_handle(stream)))
    return res

  def inverse(self, qacc, out=None, stream=None):
    """(B, nv) = mj_rne(flg_acc=1) = M qacc + bias(): the joint forces that produce `qacc` ((B, nv), or (nv,) for every
    environment) against the rigid-body terms alone.  This is mj_rne, NOT mj_inverse: passive, actuator and constraint
    forces are not part of it.  One launch; `out` and `stream` as in `mass_matrix`."""
    _, _, dt = self._torch()
    B, nv = self.batch.batch_size, self.nv
    a = self._input(qacc, ((B, nv), (nv,)), 'qacc')
    res = self._tensor((B, nv), dt, out)
    _native.check(_native.lib().dmc_dyn_inverse(self._ptr, a.data_ptr(), nv if a.dim() == 2 else 0, res.data_ptr(), self.stream_handle(stream)))
    self._keep = a      # (alive until the next call: the launch is asynchronous)
    return res

  def _vectors(self, call, x, what, out, stream):
    _, _, dt = self._torch()
    B, nv = self.batch.batch_size, self.nv
    v = self._input(x, ((B, nv), (B, None, nv)), what)
    res = self._tensor(tuple(v.shape), dt, out)
    _native.check(call(self._ptr, v.data_ptr(), 1 if v.dim() == 2 else int(v.shape[1]), res.data_ptr(), self.stream_handle(stream)))
    self._keep = v
    return res

  def mul(self, v, out=None, stream=None):
    """M v (mj_mulM): v (B, nv) -> (B, nv), or (B, K, nv) -> (B, K, nv).  One launch; `out` and `stream` as in
    `mass_matrix`."""
    return self._vectors(_native.lib().dmc_dyn_mul, v, 'v', out, stream)

  def solve(self, f, out=None, stream=None):
    """x = M^-1 f (mj_solveM): f (B, nv) -> (B, nv), or (B, K, nv) -> (B, K, nv); the K right-hand sides of an environment
    share one Cholesky factorisation.  A pivot below mjMINVAL is replaced by it.  One launch; `out` and `stream` as in
    `mass_matrix`."""
    return self._vectors(_native.lib().dmc_dyn_solve, f, 'f', out, stream)

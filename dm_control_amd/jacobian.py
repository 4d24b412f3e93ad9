"""BatchJacobian: the mj_jac family, mj_objectVelocity and the joint forces of a Cartesian wrench for a whole batch, each
computed on the device by one HIP launch.

The reference asks one point of one environment per call (`mujoco.mj_jac`, `mj_jacBody`, `mj_jacBodyCom`, `mj_jacSite`,
`mj_jacGeom`, `mj_objectVelocity`: mujoco/wrapper/core.py:522, utils/inverse_kinematics.py:179).  This module gives a
batch the same numbers as tensors that never leave the GPU:

  * a target is a point that moves with a body: a site name (a bare string), `dict(site=..)`, `dict(body=..)` (the frame
    origin, xpos), `dict(body=.., com=True)` (xipos), `dict(geom=..)` or `dict(body=.., offset=(x, y, z))` with the offset in
    the body's frame.  Names or ids.
  * jac():       jacp, jacr (B, T, 3, C): the translational and rotational Jacobian of every target; C = all dofs of
                 `joint_names`, in that order, or every dof of the model.  Columns of dofs off a target's chain are zero.
  * velocity():  (B, T, 6) = J qvel over ALL dofs, (angular, linear) as mj_objectVelocity orders them, in the world frame
                 or (`local`) the target's own -- the site's, the geom's, the body's or the inertial frame.
  * force():     (B, C) = sum over targets of jacp' force + jacr' torque: what mj_applyFT adds to a qfrc vector.

The kinematics are computed along each target's chain from the qpos in device memory (csrc/jac_core.h): the result is
mj_jac after mj_kinematics at the CURRENT qpos.  No pose array is read, so the unit needs no output mask and can never
read stale poses.  The chains are read from the compiled model when the object is made: model edits made afterwards
(body_pos, site_pos, ...) need a new object.  A target below a mocap body is refused: its pose is not a function of qpos.

Column conventions (host_data.dof_axes): a free joint has world translation axes and body-local rotation axes; a ball
joint has the columns of the body's orientation about the joint's anchor.
"""
import ctypes

import numpy as np

from dm_control_amd import _native
from dm_control_amd import _unit

MAX_CHAIN_DOFS = 64
KINDS = ('site', 'body', 'com', 'geom', 'offset')
_JNT_NQ, _JNT_NV = (7, 4, 1, 1), (6, 3, 1, 1)
_INT_TABLES = ('body_jntadr', 'body_jntnum', 'jnt_type', 'jnt_qadr', 'jnt_dslot', 'dof_id', 'dof_col')
_REAL_TABLES = ('body_pos', 'body_quat', 'jnt_axis', 'jnt_pos', 'jnt_qpos0', 'target_pos', 'target_quat')


class _Tables(ctypes.Structure):      # dmc_jac_tables
  _fields_ = [('ntarget', ctypes.c_int32), ('ncol', ctypes.c_int32), ('nints', ctypes.c_int32), ('nreals', ctypes.c_int32),
              ('dims', ctypes.c_void_p), ('ints', ctypes.c_void_p), ('reals', ctypes.c_void_p)]


def _id(model, key, kind, count):
  if isinstance(key, str):
    return int(model.name2id(key, kind))      # (ValueError: no such name)
  if isinstance(key, (int, np.integer)) and not isinstance(key, bool):
    if not 0 <= int(key) < count:
      raise ValueError('target: %s id %d out of range (the model has %d)' % (kind, int(key), count))
    return int(key)
  raise ValueError('target: a %s is named by a string or an id, got %r' % (kind, key))


def resolve_target(model, target):
  """dict(kind, id, body, pos (3,), quat (4,)) of a target: the body it moves with and its frame in that body's."""
  m = model
  if isinstance(target, str):
    target = dict(site=target)
  if not isinstance(target, dict):
    raise ValueError('target: expected a site name or dict(site= | body= | geom= ..), got %r' % (target,))
  keys = set(target)
  f64 = lambda a: np.array(a, dtype=np.float64)
  ident = np.array([1.0, 0, 0, 0])
  if keys == {'site'}:
    i = _id(m, target['site'], 'site', m.nsite)
    return dict(kind='site', id=i, body=int(m.site_bodyid[i]), pos=f64(m.site_pos[i]), quat=f64(m.site_quat[i]))
  if keys == {'geom'}:
    i = _id(m, target['geom'], 'geom', m.ngeom)
    return dict(kind='geom', id=i, body=int(m.geom_bodyid[i]), pos=f64(m.geom_pos[i]), quat=f64(m.geom_quat[i]))
  if 'body' in keys and keys <= {'body', 'com', 'offset'}:
    b = _id(m, target['body'], 'body', m.nbody)
    if target.get('com') and 'offset' in keys:
      raise ValueError('target %r: com and offset exclude each other' % (target,))
    if target.get('com'):
      return dict(kind='com', id=b, body=b, pos=f64(m.body_ipos[b]), quat=f64(m.body_iquat[b]))
    if 'offset' in keys:
      off = np.asarray(target['offset'], dtype=np.float64)
      if off.shape != (3,) or not np.all(np.isfinite(off)):
        raise ValueError('target %r: offset must be three finite numbers' % (target,))
      return dict(kind='offset', id=b, body=b, pos=off.copy(), quat=ident.copy())
    return dict(kind='body', id=b, body=b, pos=np.zeros(3), quat=ident.copy())
  raise ValueError('target: expected a site name, dict(site=..), dict(geom=..), dict(body=..[, com=True | offset=(x, y, z)]), got %r'
                   % (target,))


def column_dofs(model, joint_names=None):
  """The model dof of every output column: every dof, or all dofs of the named joints in the order given."""
  if joint_names is None:
    return np.arange(model.nv, dtype=np.int64)
  if not isinstance(joint_names, (list, tuple, np.ndarray)):
    raise ValueError('`joint_names` must be either None, a list, a tuple, or a numpy array; got %s.' % type(joint_names))
  out = []
  for n in np.asarray(joint_names).ravel().tolist():
    j = model.name2id(str(n), 'joint')      # (ValueError: not in the model)
    d = int(model.jnt_dofadr[j])
    out.extend(range(d, d + _JNT_NV[int(model.jnt_type[j])]))
  if not out:
    raise ValueError('`joint_names` is empty: no column is left')
  if len(set(out)) != len(out):
    raise ValueError('`joint_names` names a joint twice')
  return np.asarray(out, dtype=np.int64)


def extract_chain(model, target, columns=None):
  """The chain of bodies and joints from the world to the target's body, root first, as the per-target arrays of
  `dmc_jac_tables` (include/dmc_jac.h), plus `target` (resolve_target), `bodies`, `joints`.  `columns`: the model dof of
  every output column (default: all).  utils.inverse_kinematics.extract_chain is this walk for a site; here any body
  point is a target and a chain without a joint is allowed (its Jacobian is zero)."""
  m = model
  tg = resolve_target(m, target)
  columns = np.arange(m.nv) if columns is None else np.asarray(columns)
  col_of = {int(d): k for k, d in enumerate(columns)}
  bodies, b = [], tg['body']
  while b > 0:
    bodies.append(b)
    b = int(m.body_parentid[b])
  bodies.reverse()
  mocap = np.asarray(getattr(m, 'body_mocapid', np.full(m.nbody, -1)))
  if any(int(mocap[b]) >= 0 for b in bodies):
    raise ValueError('target %r hangs off a mocap body: its pose is not a function of qpos' % (target,))
  ch = {k: [] for k in _INT_TABLES + _REAL_TABLES[:5] + ('joints',)}
  for b in bodies:
    j0, jn = int(m.body_jntadr[b]), int(m.body_jntnum[b])
    ch['body_jntadr'].append(len(ch['jnt_type']))
    ch['body_jntnum'].append(jn)
    ch['body_pos'].append(np.asarray(m.body_pos[b], dtype=np.float64))
    ch['body_quat'].append(np.asarray(m.body_quat[b], dtype=np.float64))
    for j in range(j0, j0 + jn):
      t, qa, da = int(m.jnt_type[j]), int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
      ch['joints'].append(j)
      ch['jnt_type'].append(t)
      ch['jnt_qadr'].append(qa)
      ch['jnt_dslot'].append(len(ch['dof_id']))
      ch['dof_id'].extend(range(da, da + _JNT_NV[t]))
      ch['dof_col'].extend(col_of.get(d, -1) for d in range(da, da + _JNT_NV[t]))
      ch['jnt_axis'].append(np.asarray(m.jnt_axis[j], dtype=np.float64))
      ch['jnt_pos'].append(np.asarray(m.jnt_pos[j], dtype=np.float64))
      ch['jnt_qpos0'].append(float(m.qpos0[qa]))
  if not bodies:      # a point fixed in the world: one body with no joint keeps the tables non-empty
    ch['body_jntadr'].append(0)
    ch['body_jntnum'].append(0)
    ch['body_pos'].append(np.zeros(3))
    ch['body_quat'].append(np.array([1.0, 0, 0, 0]))
  if len(ch['dof_id']) > MAX_CHAIN_DOFS:
    raise ValueError('target %r: %d dofs between the world and the target, at most %d are supported'
                     % (target, len(ch['dof_id']), MAX_CHAIN_DOFS))
  out = {k: np.ascontiguousarray(ch[k], dtype=np.int32) for k in _INT_TABLES}
  flat = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
  out.update({k: flat(ch[k]) for k in _REAL_TABLES[:5]})
  out.update(target_pos=tg['pos'], target_quat=tg['quat'], target=tg, bodies=bodies, joints=ch['joints'],
             dims=np.array([len(ch['body_jntadr']), len(ch['jnt_type']), len(ch['dof_id'])], dtype=np.int32))
  return out


def chain_tables(model, targets, joint_names=None):
  """dict(dims (T, 3) int32, ints, reals, columns, chains) of a target list: the chains concatenated as dmc_jac_create
  takes them."""
  targets = list(targets)
  if not targets:
    raise ValueError('targets: at least one target is needed')
  columns = column_dofs(model, joint_names)
  chains = [extract_chain(model, t, columns) for t in targets]
  ints = np.concatenate([np.concatenate([c[k] for k in _INT_TABLES]) for c in chains]).astype(np.int32)
  reals = np.concatenate([np.concatenate([c[k] for k in _REAL_TABLES]) for c in chains]).astype(np.float64)
  return dict(dims=np.ascontiguousarray([c['dims'] for c in chains], dtype=np.int32), ints=np.ascontiguousarray(ints),
              reals=np.ascontiguousarray(reals), columns=columns, chains=chains)


class BatchJacobian(_unit.BatchUnit):
  """Jacobians, velocities and joint forces of body points for every environment of a batch; see the module docstring.

  physics_or_batch: a `BatchedPhysics`, or anything holding one as `.batch` (Physics) or `.physics`.
  targets: a list of targets (T of them); joint_names: None (every dof) or the joints whose dofs are the columns.
  These are fixed for the object's life.  `columns` holds the model dof of every column.
  """
  _DESTROY = 'dmc_jac_destroy'
  _OUT_ERROR = 'out: expected a contiguous %s tensor of shape %s on %s'

  def __init__(self, physics_or_batch, targets, joint_names=None):
    batch = _unit.find_batch(physics_or_batch)
    if batch is None:
      raise TypeError('BatchJacobian needs a BatchedPhysics (or an object holding one as .batch / .physics / .host_physics)')
    self.batch, self.model = batch, batch.model
    self.targets = list(targets)
    self.tables = chain_tables(self.model, self.targets, joint_names)
    self.columns = self.tables['columns']
    self.output_mask = 0      # nothing a step launch writes is read: the kinematics are computed from qpos
    tb = _Tables(len(self.targets), len(self.columns), self.tables['ints'].size, self.tables['reals'].size,
                 self.tables['dims'].ctypes.data, self.tables['ints'].ctypes.data, self.tables['reals'].ctypes.data)
    self._ptr = ctypes.c_void_p()
    _native.check(_native.lib().dmc_jac_create(batch._ptr, ctypes.byref(tb), ctypes.byref(self._ptr)))
    self._keep = None

  @property
  def shape(self):
    """(B, T, C)"""
    return self.batch.batch_size, len(self.targets), len(self.columns)

  def info(self):
    a = np.zeros(10, dtype=np.int32)
    _native.check(_native.lib().dmc_jac_info(self._ptr, a.ctypes.data))
    return dict(zip(('B', 'precision', 'ntarget', 'ncol', 'block', 'column_chunk', 'lds_bytes', 'force_envs_per_block',
                     'force_lds_bytes', 'max_chain_dofs'), (int(x) for x in a)))

  def _input(self, x, shapes, what):
    """`x` as a contiguous tensor in the batch precision on the batch's device; its shape must be one of `shapes`."""
    torch, dev, dt = self._torch()
    if isinstance(x, torch.Tensor):
      if x.dtype != dt:
        raise ValueError('%s: expected dtype %s, got %s' % (what, dt, x.dtype))
      if x.device != dev:
        raise ValueError('%s: expected a tensor on %s, got %s' % (what, dev, x.device))
    else:
      a = np.asarray(x)
      if a.dtype.kind not in 'fiu':
        raise ValueError('%s: expected real numbers, got dtype %s' % (what, a.dtype))
    if tuple(np.shape(x) if not isinstance(x, torch.Tensor) else x.shape) not in shapes:
      raise ValueError('%s: expected shape %s, got %s' % (what, ' or '.join(str(s) for s in shapes), tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)))
    return (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=dt, device=dev)).contiguous()

  def jac(self, rot=True, point=None, out=None, stream=None):
    """mj_jac of every target of every environment in one launch: (jacp, jacr), each (B, T, 3, C) in the batch
    precision; rot=False: jacp alone.  point: (B, T, 3) world points that replace the targets' own -- mj_jac's general
    form, where target t only names the body.  Asynchronous on `stream` (a torch stream or a raw handle; default:
    torch's current stream), capturable in a HIP graph; `out`, a tensor (rot=False) or the pair, is written in place.
    Every element is written.  The host is never read."""
    torch, _, dt = self._torch()
    B, T, C = self.shape
    n = 2 if rot else 1
    out = [None] * n if out is None else ([out] if isinstance(out, torch.Tensor) else list(out))
    if len(out) != n:
      raise ValueError('out must hold %d tensors (jacp%s)' % (n, ', jacr' if rot else ''))
    pt = None if point is None else self._input(point, ((B, T, 3),), 'point')
    res = [self._tensor((B, T, 3, C), dt, o) for o in out]
    _native.check(_native.lib().dmc_jac_jacobian(self._ptr, pt.data_ptr() if pt is not None else None, res[0].data_ptr(),
                                                 res[1].data_ptr() if rot else None, self.stream_handle(stream)))
    self._keep = pt      # (alive until the next call: the launch is asynchronous)
    return tuple(res) if rot else res[0]

  def velocity(self, local=False, out=None, stream=None):
    """(B, T, 6): the 6D velocity (angular, linear) of every target, J qvel over all dofs of its chain, in the world frame
    or (`local`) rotated into the target's own frame -- mj_objectVelocity.  One launch; `out` and `stream` as in `jac`."""
    _, _, dt = self._torch()
    B, T, _ = self.shape
    res = self._tensor((B, T, 6), dt, out)
    _native.check(_native.lib().dmc_jac_velocity(self._ptr, int(bool(local)), res.data_ptr(), self.stream_handle(stream)))
    return res

  def force(self, force, torque=None, out=None, stream=None):
    """(B, C) = sum over targets of jacp' force + jacr' torque: the joint forces of Cartesian forces (and torques) applied
    at the targets, the joint-space image of mj_applyFT.  force / torque: (B, T, 3), (T, 3) or (3,), world frame; either may
    be None.  The targets are summed in order in plain arithmetic: two launches on the same state give equal bits.

    The result is RETURNED; the batch's qfrc_applied is not written (the facades shadow the input fields on the host: a
    device-side write would be lost or counted twice).  Apply it with

        batch.set('qfrc_applied', bj.force(f).cpu().numpy())      # through the host (C = nv), or, staying on the device,
        batch.bind('qfrc_applied', buf.data_ptr())                # once, buf an (nv, B) tensor in the batch precision,
        buf.copy_(bj.force(f).T)                                  # then before every step

    One launch; `out` and `stream` as in `jac`."""
    _, _, dt = self._torch()
    B, T, C = self.shape
    if force is None and torque is None:
      raise ValueError('force: at least one of force or torque is needed')
    shapes = ((B, T, 3), (T, 3), (3,))
    args, keep = [], []
    for x, what in ((force, 'force'), (torque, 'torque')):
      if x is None:
        args += [None, 0, 0]
        continue
      t = self._input(x, shapes, what)
      keep.append(t)
      args += [t.data_ptr(), 3*T if t.dim() == 3 else 0, 3 if t.dim() >= 2 else 0]
    res = self._tensor((B, C), dt, out)
    _native.check(_native.lib().dmc_jac_force(self._ptr, *args, res.data_ptr(), self.stream_handle(stream)))
    self._keep = keep
    return res

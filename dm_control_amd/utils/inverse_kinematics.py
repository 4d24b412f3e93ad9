"""Inverse kinematics of a site: the reference's `dm_control/utils/inverse_kinematics.py` over this backend.

`qpos_from_site_pose` keeps the reference's signature, messages and `joint_names` rules (inverse_kinematics.py:37-230):

  * on a single-environment fp64 `Physics` it is the reference's host loop -- one `forward` launch per iteration, the
    site Jacobian derived on the host (host_data.point_jacobian) -- and returns what the reference returns;
  * on a batched `Physics` the whole loop of every environment is ONE launch (`BatchIK`, csrc/ik_kernels.hip): targets
    are (3,) / (4,) or (B, 3) / (B, 4) and every field of the result has a leading B.

`BatchIK` is the device object for callers that stay on the GPU: torch tensors in and out, no host read, capturable in
a HIP graph.  It solves in the dual form, update = J' (J J' + lambda I)^-1 e (see csrc/ik_core.h and
PARITY_ASSUMPTIONS.md for where that differs from the reference's least-squares call).
"""
import collections
import ctypes
import logging

import numpy as np

from dm_control_amd import _native
from dm_control_amd import _unit
from dm_control_amd import host_data
from dm_control_amd import mjcf_compiler

_INVALID_JOINT_NAMES_TYPE = (
    '`joint_names` must be either None, a list, a tuple, or a numpy array; '
    'got {}.')
_REQUIRE_TARGET_POS_OR_QUAT = (
    'At least one of `target_pos` or `target_quat` must be specified.')

IKResult = collections.namedtuple('IKResult', ['qpos', 'err_norm', 'steps', 'success'])

CONVERGED, STEP_LIMIT, NO_PROGRESS, SINGULAR = 0, 1, 2, 3
MAX_CHAIN_DOFS = 64
TOL_F64 = 1e-14
# fp32 batches: 4 x the largest error norm at which the fp32 iteration stalls over the arm's 14 reference targets
# (5.72e-7, PARITY_ASSUMPTIONS.md "Inverse kinematics"); the factor is the margin DESIGN.md section 8 gives an fp32
# bound set from one measurement
TOL_F32_FLOOR = 5.72e-7
TOL_F32 = 4 * TOL_F32_FLOOR

_JNT_NQ, _JNT_NV = (7, 4, 1, 1), (6, 3, 1, 1)


def _joint_ids(model, joint_names):
  """None (every joint) or the ids of the named joints, by the reference's type rules (inverse_kinematics.py:139-152)."""
  if joint_names is None:
    return None
  if isinstance(joint_names, (list, np.ndarray, tuple)):
    return [model.name2id(str(n), 'joint') for n in np.asarray(joint_names).ravel().tolist()]
  raise ValueError(_INVALID_JOINT_NAMES_TYPE.format(type(joint_names)))


def _dof_indices(model, joint_ids):
  if joint_ids is None:
    return np.arange(model.nv)
  out = []
  for j in joint_ids:
    d = int(model.jnt_dofadr[j])
    out.extend(range(d, d + _JNT_NV[int(model.jnt_type[j])]))
  return np.asarray(out, dtype=np.int64)


def extract_chain(model, site_name, joint_names=None):
  """The chain of bodies and joints from the world to the site's body, root first, as the arrays of `dmc_ik_chain`
  (include/dmc_ik.h).  A snapshot of the compiled model."""
  m = model
  site = m.name2id(site_name, 'site')
  movable = _joint_ids(m, joint_names)
  bodies, b = [], int(m.site_bodyid[site])
  while b > 0:
    bodies.append(b)
    b = int(m.body_parentid[b])
  bodies.reverse()
  mocap = np.asarray(getattr(m, 'body_mocapid', np.full(m.nbody, -1)))
  if any(int(mocap[b]) >= 0 for b in bodies):
    raise ValueError('site %r hangs off a mocap body: its pose is not a function of qpos' % (site_name,))
  ch = dict(body_jntadr=[], body_jntnum=[], jnt_type=[], jnt_qslot=[], jnt_dslot=[], qmap=[], dof_movable=[], body_pos=[],
            body_quat=[], jnt_axis=[], jnt_pos=[], jnt_qpos0=[], joints=[], dofs=[])
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
      ch['jnt_qslot'].append(len(ch['qmap']))
      ch['jnt_dslot'].append(len(ch['dofs']))
      ch['qmap'].extend(range(qa, qa + _JNT_NQ[t]))
      ch['dofs'].extend(range(da, da + _JNT_NV[t]))
      ch['dof_movable'].extend([int(movable is None or j in movable)] * _JNT_NV[t])
      ch['jnt_axis'].append(np.asarray(m.jnt_axis[j], dtype=np.float64))
      ch['jnt_pos'].append(np.asarray(m.jnt_pos[j], dtype=np.float64))
      ch['jnt_qpos0'].append(float(m.qpos0[qa]))
  if not sum(ch['dof_movable']):
    raise ValueError('site %r: none of the joints that may move lies between the world and the site' % (site_name,))
  if len(ch['dofs']) > MAX_CHAIN_DOFS:
    raise ValueError('site %r: %d dofs between the world and the site, at most %d are supported'
                     % (site_name, len(ch['dofs']), MAX_CHAIN_DOFS))
  i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
  f64 = lambda a, n: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, n) if n else np.asarray(a, dtype=np.float64))
  out = {k: i32(ch[k]) for k in ('body_jntadr', 'body_jntnum', 'jnt_type', 'jnt_qslot', 'jnt_dslot', 'qmap', 'dof_movable')}
  out.update(body_pos=f64(ch['body_pos'], 3), body_quat=f64(ch['body_quat'], 4), jnt_axis=f64(ch['jnt_axis'], 3),
             jnt_pos=f64(ch['jnt_pos'], 3), jnt_qpos0=f64(ch['jnt_qpos0'], 0),
             site_pos=np.array(m.site_pos[site], dtype=np.float64), site_quat=np.array(m.site_quat[site], dtype=np.float64),
             site=site, bodies=bodies, joints=ch['joints'], dofs=np.asarray(ch['dofs'], dtype=np.int64))
  return out


class _Chain(ctypes.Structure):
  _fields_ = [('nbody', ctypes.c_int32), ('njnt', ctypes.c_int32), ('ndof', ctypes.c_int32), ('nqchain', ctypes.c_int32)] + \
      [(n, ctypes.c_void_p) for n in ('body_jntadr', 'body_jntnum', 'jnt_type', 'jnt_qslot', 'jnt_dslot', 'qmap', 'dof_movable',
                                      'body_pos', 'body_quat', 'jnt_axis', 'jnt_pos', 'jnt_qpos0')] + \
      [('site_pos', ctypes.c_double * 3), ('site_quat', ctypes.c_double * 4)]


class _Options(ctypes.Structure):
  _fields_ = [(n, ctypes.c_double) for n in ('tol', 'rot_weight', 'regularization_threshold', 'regularization_strength',
                                             'max_update_norm', 'progress_thresh')] + \
      [('max_steps', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class BatchIK(_unit.BatchUnit):
  """qpos_from_site_pose for every environment of a batch in one launch (include/dmc_ik.h).

  `physics`: a `Physics` or a `BatchedPhysics`.  The kinematic chain is read from the compiled model HERE: model edits
  made afterwards (body_pos, site_pos, ... through physics.model / set_model_real) need a new object.  Options are the
  keyword arguments of the reference's function; `tol=None` is 1e-14 on an fp64 batch and `TOL_F32` on an fp32 one."""
  _DESTROY = 'dmc_ik_destroy'

  def __init__(self, physics, site_name, joint_names=None, tol=None, rot_weight=1.0, regularization_threshold=0.1,
               regularization_strength=3e-2, max_update_norm=2.0, progress_thresh=20.0, max_steps=100):
    self.batch = getattr(physics, 'batch', physics)
    self.model = self.batch.model
    if not isinstance(self.model, mjcf_compiler.Model):
      raise TypeError('BatchIK needs a Physics or BatchedPhysics built from a compiled Model')
    self.chain = extract_chain(self.model, site_name, joint_names)
    self.precision = int(self.batch.precision)
    self.tol = float((TOL_F64 if self.precision == 64 else TOL_F32) if tol is None else tol)
    self.max_steps = int(max_steps)
    c, ch = _Chain(), self.chain
    c.nbody, c.njnt, c.ndof, c.nqchain = len(ch['body_jntadr']), len(ch['jnt_type']), len(ch['dofs']), len(ch['qmap'])
    for n in ('body_jntadr', 'body_jntnum', 'jnt_type', 'jnt_qslot', 'jnt_dslot', 'qmap', 'dof_movable', 'body_pos', 'body_quat',
              'jnt_axis', 'jnt_pos', 'jnt_qpos0'):
      setattr(c, n, ch[n].ctypes.data)
    c.site_pos[:], c.site_quat[:] = list(ch['site_pos']), list(ch['site_quat'])
    o = _Options(self.tol, float(rot_weight), float(regularization_threshold), float(regularization_strength),
                 float(max_update_norm), float(progress_thresh), self.max_steps, 0)
    self._ptr = ctypes.c_void_p()
    L = _native.lib()
    if L.dmc_ik_create(self.batch._ptr, ctypes.byref(c), ctypes.byref(o), ctypes.byref(self._ptr)) != 0:
      raise _native.NativeError(L.dmc_ik_last_error().decode())

  def info(self):
    a = np.zeros(7, dtype=np.int32)
    if _native.lib().dmc_ik_info(self._ptr, a.ctypes.data) != 0:
      raise _native.NativeError(_native.lib().dmc_ik_last_error().decode())
    return dict(zip(('B', 'precision', 'envs_per_block', 'lds_bytes_per_block', 'grid', 'ndof', 'nqchain'), (int(x) for x in a)))

  def _target(self, t, n, torch, dev, dt):
    if t is None:
      return None
    B = self.batch.batch_size
    t = torch.as_tensor(t, dtype=dt, device=dev) if not isinstance(t, torch.Tensor) else t.to(device=dev, dtype=dt)
    if tuple(t.shape) not in ((n,), (B, n)):
      raise ValueError('target must have shape (%d,) or (%d, %d), got %s' % (n, B, n, tuple(t.shape)))
    return t.expand(B, n).contiguous()

  def solve(self, target_pos=None, target_quat=None, qpos=None, inplace=False, stream=None):
    """Returns dict(qpos (B, nq), err_norm (B,), steps (B,) int32, status (B,) int32) of torch tensors on the batch's
    device; `success` is `status == 0`.  `qpos=None` starts from the batch's own qpos; `inplace=True` also writes the
    result there (and invalidates the batch's stashes on the stream).  Asynchronous on `stream` (a torch stream or a raw
    handle; default: torch's current stream)."""
    if target_pos is None and target_quat is None:
      raise ValueError(_REQUIRE_TARGET_POS_OR_QUAT)
    torch, dev, dt = self._torch()
    B, nq = self.batch.batch_size, int(self.model.nq)
    tp, tq = self._target(target_pos, 3, torch, dev, dt), self._target(target_quat, 4, torch, dev, dt)
    if qpos is not None:
      qpos = torch.as_tensor(qpos, dtype=dt, device=dev) if not isinstance(qpos, torch.Tensor) else qpos.to(device=dev, dtype=dt)
      if tuple(qpos.shape) != (B, nq):
        raise ValueError('qpos must have shape (%d, %d), got %s' % (B, nq, tuple(qpos.shape)))
      qpos = qpos.contiguous()
    out = dict(qpos=self._tensor((B, nq), dt), err_norm=self._tensor((B,), dt), steps=self._tensor((B,), torch.int32),
               status=self._tensor((B,), torch.int32))
    ptr = lambda t: t.data_ptr() if t is not None else None
    L = _native.lib()
    if L.dmc_ik_solve(self._ptr, ptr(tp), ptr(tq), ptr(qpos), int(bool(inplace)), out['qpos'].data_ptr(),
                      out['err_norm'].data_ptr(), out['steps'].data_ptr(), out['status'].data_ptr(), self.stream_handle(stream)) != 0:
      raise _native.NativeError(L.dmc_ik_last_error().decode())
    self._keep = (tp, tq, qpos)      # (alive until the next solve: the launch is asynchronous)
    return out


def _quat2vel(q):
  axis = np.array(q[1:4], dtype=np.float64)
  s = np.linalg.norm(axis)
  axis = axis / s if s >= host_data.MINVAL else np.array([1.0, 0, 0])
  speed = 2 * np.arctan2(s, q[0])
  if speed > np.pi:
    speed -= 2 * np.pi
  return axis * speed


def _site_jacobian(physics, site_id):
  m, d = physics.model, physics.data
  xpos, xquat = np.asarray(d.xpos, dtype=np.float64), np.asarray(d.xquat, dtype=np.float64)
  anchor, axis = host_data.joint_frames(m, np.asarray(physics.batch.get('qpos'), dtype=np.float64)[0], xpos, xquat)
  return host_data.point_jacobian(m, int(m.site_bodyid[site_id]), np.asarray(d.site_xpos, dtype=np.float64)[site_id], xpos,
                                  host_data.quat_to_mat_rows(xquat), anchor, axis)


def _host_loop(physics, site_id, target_pos, target_quat, dof_indices, tol, rot_weight, regularization_threshold,
               regularization_strength, max_update_norm, progress_thresh, max_steps):
  """inverse_kinematics.py:157-214 on one environment: a forward launch per iteration."""
  m = physics.model
  update_nv = np.zeros(m.nv)
  physics.forward()
  steps, success, err_norm = 0, False, 0.0
  for steps in range(max_steps):
    err, err_norm = [], 0.0
    if target_pos is not None:
      e = np.asarray(target_pos, dtype=np.float64) - np.asarray(physics.data.site_xpos, dtype=np.float64)[site_id]
      err.append(e)
      err_norm += np.linalg.norm(e)
    if target_quat is not None:
      xquat = mjcf_compiler.mat_to_quat(np.asarray(physics.data.site_xmat, dtype=np.float64)[site_id].reshape(3, 3))
      e = _quat2vel(mjcf_compiler.quat_mul(np.asarray(target_quat, dtype=np.float64), xquat * np.array([1.0, -1, -1, -1])))
      err.append(e)
      err_norm += np.linalg.norm(e) * rot_weight
    if err_norm < tol:
      success = True
      break
    jp, jr = _site_jacobian(physics, site_id)
    jac = np.concatenate(([jp] if target_pos is not None else []) + ([jr] if target_quat is not None else []))
    reg = regularization_strength if err_norm > regularization_threshold else 0.0
    update = nullspace_method(jac[:, dof_indices], np.concatenate(err), regularization_strength=reg)
    update_norm = np.linalg.norm(update)
    with np.errstate(divide='ignore', invalid='ignore'):
      progress = err_norm / update_norm
    if progress > progress_thresh:
      break
    if update_norm > max_update_norm:
      update = update * (max_update_norm / update_norm)
    update_nv[dof_indices] = update
    qpos = np.array(physics.data.qpos, dtype=np.float64)
    host_data.integrate_pos(m, qpos, update_nv, 1.0)
    physics.data.qpos = qpos
    physics.forward()
  if not success and steps == max_steps - 1:
    logging.getLogger(__name__).warning('Failed to converge after %i steps: err_norm=%3g', steps, err_norm)
  return err_norm, steps, success


def qpos_from_site_pose(physics, site_name, target_pos=None, target_quat=None, joint_names=None, tol=None, rot_weight=1.0,
                        regularization_threshold=0.1, regularization_strength=3e-2, max_update_norm=2.0,
                        progress_thresh=20.0, max_steps=100, inplace=False):
  """Joint positions that put a site at a target position and / or orientation: the reference's function
  (inverse_kinematics.py:37-230), same arguments and `IKResult(qpos, err_norm, steps, success)`.

  `tol=None` is the reference's 1e-14 on fp64 and `TOL_F32` on an fp32 batch.  On a batched `Physics` the targets are
  (3,) / (4,) or (B, 3) / (B, 4), every result field has a leading B, and the solve runs on the device (`BatchIK`)."""
  if target_pos is None and target_quat is None:
    raise ValueError(_REQUIRE_TARGET_POS_OR_QUAT)
  model = physics.model
  joint_ids = _joint_ids(model, joint_names)
  opts = dict(rot_weight=rot_weight, regularization_threshold=regularization_threshold,
              regularization_strength=regularization_strength, max_update_norm=max_update_norm,
              progress_thresh=progress_thresh, max_steps=max_steps)
  if physics.batch_size > 1 or int(physics.batch.precision) != 64:
    physics.data._upload()      # (host writes to physics.data that have not reached the device yet)
    ik = BatchIK(physics, site_name, joint_names, tol=tol, **opts)
    try:
      out = ik.solve(target_pos, target_quat, inplace=inplace)
      res = {k: v.cpu().numpy() for k, v in out.items()}
    finally:
      ik.close()
    if inplace:
      physics.data._invalidate()
    qpos, err, steps, ok = res['qpos'].astype(np.float64), res['err_norm'].astype(np.float64), res['steps'], res['status'] == CONVERGED
    if physics.batch_size == 1:
      return IKResult(qpos=qpos[0], err_norm=float(err[0]), steps=int(steps[0]), success=bool(ok[0]))
    return IKResult(qpos=qpos, err_norm=err, steps=steps, success=ok)
  site_id = model.name2id(site_name, 'site')
  if not inplace:
    physics = physics.copy(share_model=True)
  err_norm, steps, success = _host_loop(physics, site_id, target_pos, target_quat, _dof_indices(model, joint_ids),
                                        TOL_F64 if tol is None else tol, **opts)
  qpos = np.array(physics.data.qpos, dtype=np.float64) if not inplace else physics.data.qpos
  if not inplace:
    physics.free()
  return IKResult(qpos=qpos, err_norm=err_norm, steps=steps, success=success)


def nullspace_method(jac_joints, delta, regularization_strength=0.0):
  """The joint update for an end-effector delta (inverse_kinematics.py:233-260): damped least squares
  (J'J + lambda I)^-1 J' delta for lambda > 0, the minimum-norm least-squares solution otherwise."""
  jac = np.asarray(jac_joints)
  rhs = jac.T @ np.asarray(delta)
  normal = jac.T @ jac
  if regularization_strength > 0:
    normal[np.diag_indices_from(normal)] += regularization_strength
    return np.linalg.solve(normal, rhs)
  return np.linalg.lstsq(normal, rhs, rcond=-1)[0]

"""TEST INFRASTRUCTURE: a plain-numpy fp64 restatement of batched inverse kinematics, written from the algorithm's
description (chain kinematics, site Jacobian, dual damped least squares, mj_integratePos) and sharing no code with the
package.  It reads a compiled model's arrays and nothing else.

One environment at a time:

  twin = Twin(model, 'gripsite', joint_names)
  pos, quat = twin.site_pose(qpos)
  jp, jr = twin.jacobian(qpos)                      # (3, nv) each
  out = twin.solve(qpos, target_pos, target_quat)   # dict(qpos, err_norm, steps, status, trace)

`status`: 0 converged, 1 step limit, 2 progress stop, 3 singular pivot.  `trace`: per iteration (err_norm, progress
ratio or None), for tests that must know how close a decision came to its threshold."""
import numpy as np

FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3
TINY = 1e-15


def qmul(a, b):
  return np.array([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3],
                   a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                   a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1],
                   a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]])


def qmat(q):
  w, x, y, z = q
  return np.array([[w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y)],
                   [2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x)],
                   [2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z]])


def qunit(q):
  n = np.linalg.norm(q)
  if n < TINY:
    return np.array([1.0, 0, 0, 0])
  return q / n if abs(n - 1) > TINY else np.array(q, dtype=np.float64)


def unit3(v):
  n = np.linalg.norm(v)
  return (v / n, n) if n >= TINY else (np.array([1.0, 0, 0]), n)


def quat_to_vel(q):
  axis, s = unit3(np.array(q[1:4], dtype=np.float64))
  speed = 2*np.arctan2(s, q[0])
  if speed > np.pi:
    speed -= 2*np.pi
  return axis*speed


def quat_step(q, v):
  """q turned by the local rotation vector v."""
  axis, n = unit3(np.array(v, dtype=np.float64))
  return qmul(qunit(q), np.concatenate([[np.cos(n/2)], axis*np.sin(n/2)]))


class Twin:

  def __init__(self, model, site_name, joint_names=None):
    m = self.m = model
    self.site = m.names['site'].index(site_name)
    chain, b = [], int(m.site_bodyid[self.site])
    while b > 0:
      chain.append(b)
      b = int(m.body_parentid[b])
    self.bodies = chain[::-1]
    names = None if joint_names is None else [str(n) for n in joint_names]
    self.movable = np.zeros(m.nv, dtype=bool)
    for b in self.bodies:
      for j in range(int(m.body_jntadr[b]), int(m.body_jntadr[b]) + int(m.body_jntnum[b])):
        if names is None or m.names['joint'][j] in names:
          d = int(m.jnt_dofadr[j])
          self.movable[d:d + (6, 3, 1, 1)[int(m.jnt_type[j])]] = True

  # -- kinematics: returns site pose and, per dof of the chain, (axis, anchor, rotates) -----------------------------
  def _walk(self, qpos):
    m = self.m
    pos, quat = np.zeros(3), np.array([1.0, 0, 0, 0])
    cols = {}
    for b in self.bodies:
      j0, jn = int(m.body_jntadr[b]), int(m.body_jntnum[b])
      pending = []
      if jn == 1 and int(m.jnt_type[j0]) == FREE:
        a, d = int(m.jnt_qposadr[j0]), int(m.jnt_dofadr[j0])
        pos, quat = np.array(qpos[a:a + 3], dtype=np.float64), qunit(np.asarray(qpos[a + 3:a + 7], dtype=np.float64))
        pending.append((FREE, d, None))
      else:
        pos = pos + qmat(quat) @ np.asarray(m.body_pos[b], dtype=np.float64)
        quat = qmul(quat, np.asarray(m.body_quat[b], dtype=np.float64))
        for j in range(j0, j0 + jn):
          t, a, d = int(m.jnt_type[j]), int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
          R = qmat(quat)
          anchor = pos + R @ np.asarray(m.jnt_pos[j], dtype=np.float64)
          axis = R @ np.asarray(m.jnt_axis[j], dtype=np.float64)
          if t == SLIDE:
            pos = pos + axis*(qpos[a] - m.qpos0[a])
            cols[d] = (axis, anchor, False)
            continue
          if t == HINGE:
            ang = qpos[a] - m.qpos0[a]
            ql = np.concatenate([[np.cos(ang/2)], np.asarray(m.jnt_axis[j], dtype=np.float64)*np.sin(ang/2)])
            cols[d] = (axis, anchor, True)
          else:
            ql = qunit(np.asarray(qpos[a:a + 4], dtype=np.float64))
            pending.append((BALL, d, anchor))
          quat = qmul(quat, ql)
          pos = anchor - qmat(quat) @ np.asarray(m.jnt_pos[j], dtype=np.float64)
      quat = qunit(quat)
      R = qmat(quat)
      for t, d, anchor in pending:
        if t == BALL:
          for i in range(3):
            cols[d + i] = (R[:, i].copy(), anchor, True)
        else:
          for i in range(3):
            cols[d + i] = (np.eye(3)[i], pos.copy(), False)
            cols[d + 3 + i] = (R[:, i].copy(), pos.copy(), True)
    spos = pos + qmat(quat) @ np.asarray(m.site_pos[self.site], dtype=np.float64)
    squat = qmul(quat, np.asarray(m.site_quat[self.site], dtype=np.float64))
    return spos, squat, cols

  def site_pose(self, qpos):
    spos, squat, _ = self._walk(qpos)
    return spos, squat

  def jacobian(self, qpos):
    spos, _, cols = self._walk(qpos)
    jp, jr = np.zeros((3, self.m.nv)), np.zeros((3, self.m.nv))
    for d, (axis, anchor, rot) in cols.items():
      if rot:
        jp[:, d], jr[:, d] = np.cross(axis, spos - anchor), axis
      else:
        jp[:, d] = axis
    return jp, jr

  def integrate(self, qpos, v):
    m, q = self.m, np.array(qpos, dtype=np.float64)
    for j in range(m.njnt):
      t, a, d = int(m.jnt_type[j]), int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
      if not self.movable[d]:
        continue
      if t == FREE:
        q[a:a + 3] += v[d:d + 3]
        q[a + 3:a + 7] = quat_step(q[a + 3:a + 7], v[d + 3:d + 6])
      elif t == BALL:
        q[a:a + 4] = quat_step(q[a:a + 4], v[d:d + 3])
      else:
        q[a] += v[d]
    return q

  def error(self, qpos, target_pos, target_quat, rot_weight=1.0):
    spos, squat = self.site_pose(qpos)
    e, n = [], 0.0
    if target_pos is not None:
      ep = np.asarray(target_pos, dtype=np.float64) - spos
      e.append(ep)
      n += np.linalg.norm(ep)
    if target_quat is not None:
      er = quat_to_vel(qmul(np.asarray(target_quat, dtype=np.float64), squat*np.array([1.0, -1, -1, -1])))
      e.append(er)
      n += np.linalg.norm(er)*rot_weight
    return np.concatenate(e), n

  def solve(self, qpos, target_pos=None, target_quat=None, tol=1e-14, rot_weight=1.0, regularization_threshold=0.1,
            regularization_strength=3e-2, max_update_norm=2.0, progress_thresh=20.0, max_steps=100):
    q = np.array(qpos, dtype=np.float64)
    status, steps, en, trace = 1, max_steps - 1, 0.0, []
    for it in range(max_steps):
      e, en = self.error(q, target_pos, target_quat, rot_weight)
      if en < tol:
        status, steps = 0, it
        trace.append((en, None))
        break
      jp, jr = self.jacobian(q)
      J = np.concatenate(([jp] if target_pos is not None else []) + ([jr] if target_quat is not None else []))[:, self.movable]
      A = J @ J.T
      if en > regularization_threshold:
        A = A + regularization_strength*np.eye(len(e))
      try:
        L = np.linalg.cholesky(A)
      except np.linalg.LinAlgError:
        status, steps = 3, it
        trace.append((en, None))
        break
      y = np.linalg.solve(L.T, np.linalg.solve(L, e))
      u = J.T @ y
      un = np.linalg.norm(u)
      with np.errstate(divide='ignore', invalid='ignore'):
        ratio = en/un
      trace.append((en, ratio))
      if ratio > progress_thresh:
        status, steps = 2, it
        break
      if un > max_update_norm:
        u = u*(max_update_norm/un)
      v = np.zeros(self.m.nv)
      v[self.movable] = u
      q = self.integrate(q, v)
    return dict(qpos=q, err_norm=en, steps=steps, status=status, trace=trace)

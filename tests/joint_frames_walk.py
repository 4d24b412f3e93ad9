"""TEST INFRASTRUCTURE: mjData.xanchor / xaxis by mj_kinematics' own forward walk, one environment and one joint at a
time -- the independent restatement the vectorised backward walk of `dm_control_amd.host_data.joint_frames` is compared
with.  Each joint's anchor and axis are taken in the body frame accumulated BEFORE that joint moves it, starting from the
parent's frame, so bodies with several joints cannot be served from the final xpos / xmat.
"""
import numpy as np

from dm_control_amd import mjcf_compiler


def joint_frames_walk(model, qpos, xpos, xquat, mocap_pos=None, mocap_quat=None):
  """(anchor, axis), each (B, njnt, 3), from qpos (B, nq), xpos (B, nbody, 3), xquat (B, nbody, 4) and, for a model with
  mocap bodies, mocap_pos (B, nmocap, 3) / mocap_quat (B, nmocap, 4)."""
  m = model
  qpos = np.asarray(qpos, dtype=np.float64)
  B = qpos.shape[0]
  xpos = np.asarray(xpos, dtype=np.float64).reshape(B, -1, 3)
  xquat = np.asarray(xquat, dtype=np.float64).reshape(B, -1, 4)
  mpos = np.asarray(mocap_pos, dtype=np.float64).reshape(B, -1, 3) if getattr(m, 'nmocap', 0) else None
  mquat = np.asarray(mocap_quat, dtype=np.float64).reshape(B, -1, 4) if getattr(m, 'nmocap', 0) else None
  C = mjcf_compiler
  anchor, axis = np.zeros((B, m.njnt, 3)), np.zeros((B, m.njnt, 3))
  for e in range(B):
    for b in range(1, m.nbody):
      j0, jn = int(m.body_jntadr[b]), int(m.body_jntnum[b])
      if jn == 0:
        continue
      if jn == 1 and m.jnt_type[j0] == 0:      # free joint
        qa = int(m.jnt_qposadr[j0])
        anchor[e, j0] = qpos[e, qa:qa + 3]
        axis[e, j0] = m.jnt_axis[j0]
        continue
      pid = int(m.body_parentid[b])
      bp, bq = m.body_pos[b], m.body_quat[b]
      if getattr(m, 'nmocap', 0) and m.body_mocapid[b] >= 0:
        bp, bq = mpos[e, m.body_mocapid[b]], mquat[e, m.body_mocapid[b]] / np.linalg.norm(mquat[e, m.body_mocapid[b]])
      pos = xpos[e, pid] + C.quat_to_mat(xquat[e, pid]) @ bp if pid else np.array(bp, dtype=np.float64)
      quat = C.quat_mul(xquat[e, pid], bq) if pid else np.array(bq, dtype=np.float64)
      for j in range(j0, j0 + jn):
        R = C.quat_to_mat(quat)
        axis[e, j] = R @ m.jnt_axis[j]
        anchor[e, j] = R @ m.jnt_pos[j] + pos
        qa, t = int(m.jnt_qposadr[j]), int(m.jnt_type[j])
        if t == 2:      # slide
          pos = pos + axis[e, j] * (qpos[e, qa] - m.qpos0[qa])
        else:           # ball / hinge: rotate about the anchor
          if t == 1:
            qloc = qpos[e, qa:qa + 4] / np.linalg.norm(qpos[e, qa:qa + 4])
          else:
            qloc = C.axisangle_to_quat(m.jnt_axis[j], qpos[e, qa] - m.qpos0[qa])
          quat = C.quat_mul(quat, qloc)
          pos = anchor[e, j] - C.quat_to_mat(quat) @ m.jnt_pos[j]
  return anchor, axis

"""TEST INFRASTRUCTURE: the fp64 twin of the contact-wrench unit, plain numpy loops written from the definition
(PARITY_ASSUMPTIONS rows 82-87) over ONE environment's contact list.  It shares no code with dm_control_amd: sets of geoms
are Python sets, a contact is a dict.

  contacts: a list of dict(geom1, geom2, dist, pos (3,), frame (3, 3) rows normal / tangent / tangent, force (6,) in the
            contact frame)
  target:   dict(S=set of geom ids, O=set of geom ids or None (every geom), r=(3,) the point the torque is taken about,
            R=(3, 3) the named body's orientation or None (world frame))
"""
import numpy as np


def world_wrench(c):
  """(f, t): the force on geom2's body and the torque about the contact point, in the world frame."""
  F, lf = np.asarray(c['frame'], dtype=np.float64).reshape(3, 3), np.asarray(c['force'], dtype=np.float64).reshape(6)
  f, t = np.zeros(3), np.zeros(3)
  for k in range(3):
    for j in range(3):
      f[k] += F[j, k] * lf[j]
      t[k] += F[j, k] * lf[3 + j]
  return f, t


def sign(c, S, O):
  g1, g2 = int(c['geom1']), int(c['geom2'])
  in_o = lambda g: O is None or g in O
  if g2 in S and in_o(g1) and g1 not in S:
    return 1
  if g1 in S and in_o(g2) and g2 not in S:
    return -1
  return 0


def wrench(contacts, nconmax):
  out = np.zeros((nconmax, 6))
  for i, c in enumerate(contacts):
    out[i, :3], out[i, 3:] = world_wrench(c)
  return out


def net(contacts, target):
  """dict(force, torque (3,), normal, dist, count, signs (the sign of every contact, 0: not counted))."""
  S, O, r, R = target['S'], target.get('O'), np.asarray(target['r'], dtype=np.float64), target.get('R')
  force, torque, normal, dist, count, signs = np.zeros(3), np.zeros(3), 0.0, np.inf, 0, []
  for c in contacts:
    s = sign(c, S, O)
    signs.append(s)
    if not s:
      continue
    f, t = world_wrench(c)
    d = np.asarray(c['pos'], dtype=np.float64) - r
    lever = np.array([d[1]*f[2] - d[2]*f[1], d[2]*f[0] - d[0]*f[2], d[0]*f[1] - d[1]*f[0]])
    force += s * f
    torque += s * (t + lever)
    normal += float(np.asarray(c['force']).reshape(6)[0])
    dist = min(dist, float(c['dist']))
    count += 1
  if R is not None:
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    force, torque = R.T @ force, R.T @ torque
  return dict(force=force, torque=torque, normal=normal, dist=dist, count=count, signs=signs)

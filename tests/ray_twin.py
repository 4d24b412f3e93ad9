"""TEST INFRASTRUCTURE: a plain-numpy fp64 mj_ray over the project's filter rules, written from the specification
(PARITY_ASSUMPTIONS.md rows 58-60) and independent of the kernels; the per-primitive closed forms are the camera twin's
(camera_twin.ray_geom, textbook discriminant).

One ray pnt + x vec: the smallest x >= 0, in units of |vec|, over the geoms that pass the filter, and that geom's id;
-1 / -1 when nothing is hit.  Skipped: geoms on body `bodyexclude`, invisible geoms, geoms whose group's flag (clamped to
0..5) is zero, with flg_static 0 the geoms of bodies welded to the world, meshes and height fields.

The edge rule: a ray is excluded from comparison when the twin changes hit geom, or changes distance by more than 1 %,
under a perturbation of the direction by +-1e-3 |vec| along either of two unit vectors perpendicular to vec.
"""
import numpy as np

import camera_twin as twin

PROBE = 1e-3


def hittable(model, geomgroup=None, flg_static=1):
  ok = np.zeros(model.ngeom, dtype=bool)
  for g in range(model.ngeom):
    if int(model.geom_type[g]) not in twin.DRAWN or model.geom_invisible[g]:
      continue
    if geomgroup is not None and not geomgroup[min(5, max(0, int(model.geom_group[g])))]:
      continue
    if not flg_static and int(model.body_weldid[int(model.geom_bodyid[g])]) == 0:
      continue
    ok[g] = True
  return ok


def perpendiculars(vec):
  """Two unit vectors perpendicular to each row of vec (N, 3) and to each other."""
  v = vec / np.linalg.norm(vec, axis=1, keepdims=True)
  e = np.eye(3)[np.argmin(np.abs(v), axis=1)]
  u1 = np.cross(v, e)
  u1 /= np.linalg.norm(u1, axis=1, keepdims=True)
  return u1, np.cross(v, u1)


def probes(vec):
  """(N, 5, 3): each direction and its four perturbations."""
  u1, u2 = perpendiculars(vec)
  h = PROBE * np.linalg.norm(vec, axis=1, keepdims=True)
  return np.stack([vec, vec + h*u1, vec - h*u1, vec + h*u2, vec - h*u2], 1)


def cast(model, geom_xpos, geom_xmat, pnt, vec, bodyexclude=-1, geomgroup=None, flg_static=1, cutoff=None, geom_size=None,
         edge=True):
  """pnt, vec (N, 3); bodyexclude one id or (N).  Returns dict(dist (N), gid (N), normal (N, 3) world frame, excluded (N)
  bool -- all False with edge=False)."""
  pnt = np.asarray(pnt, dtype=np.float64).reshape(-1, 3)
  vec = np.asarray(vec, dtype=np.float64).reshape(-1, 3)
  N = len(vec)
  bex = np.broadcast_to(np.asarray(bodyexclude), (N,))
  gpos = np.asarray(geom_xpos, dtype=np.float64).reshape(-1, 3)
  gmat = np.asarray(geom_xmat, dtype=np.float64).reshape(-1, 3, 3)
  size = np.asarray(model.geom_size if geom_size is None else geom_size, dtype=np.float64).reshape(-1, 3)
  ok = hittable(model, geomgroup, flg_static)
  dirs = probes(vec) if edge else vec[:, None]
  P = dirs.shape[1]
  best = np.full((N, P), np.inf)
  gid = np.full((N, P), -1)
  normal = np.zeros((N, 3))
  for i in range(N):
    length = np.linalg.norm(dirs[i], axis=1)
    for g in np.nonzero(ok)[0]:
      if int(model.geom_bodyid[g]) == int(bex[i]):
        continue
      Rg = gmat[g]
      t, n = twin.ray_geom(int(model.geom_type[g]), size[g], Rg.T @ (pnt[i] - gpos[g]), dirs[i] @ Rg)
      if cutoff is not None:
        t = np.where(t * length > cutoff, np.inf, t)
      m = t < best[i]
      best[i] = np.where(m, t, best[i])
      gid[i] = np.where(m, g, gid[i])
      if m[0]:
        normal[i] = Rg @ n[0]
  d0, g0 = best[:, 0], gid[:, 0]
  ex = np.zeros(N, dtype=bool)
  for k in range(1, P):
    with np.errstate(all='ignore'):
      rel = np.abs(best[:, k] - d0) / np.maximum(np.abs(d0), twin.MINVAL)
    ex |= (gid[:, k] != g0) | ((g0 >= 0) & (rel > 0.01))
  return dict(dist=np.where(g0 >= 0, d0, -1.0), gid=g0, normal=normal, excluded=ex)

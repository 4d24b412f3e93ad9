"""TEST INFRASTRUCTURE: a plain-numpy fp64 restatement of the geometric camera (camera poses, pinhole rays, nearest
hit, surface normals, headlight shading), written from the camera's specification and independent of the kernel.

Pinhole: f = 0.5 H / tan(fovy / 2); pixel (r, c), row 0 at the top, looks along the camera-frame direction
((c - (W - 1) / 2) / f, -(r - (H - 1) / 2) / f, -1); with that unnormalised direction the ray parameter of the nearest
hit is the depth along the optical axis.  Rays are the rangefinder's: planes front-side only and finite where their
half-sizes are positive; a ray that starts inside a solid leaves through its surface.
"""
import math

import numpy as np

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = 0, 2, 3, 4, 5, 6
DRAWN = (PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX)
MINVAL = 1e-15


def quat_to_mat(q):
  w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
  return np.array([[1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y)],
                   [2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x)],
                   [2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)]])


def camera_pose(mode, body, target, pos, quat, pos0, poscom0, mat0, xpos, xmat, com):
  """World (position, 3x3 orientation) of one camera of one environment.  xpos (nbody, 3), xmat (nbody, 3, 3), com
  (nbody, 3)."""
  if mode == 1:
    return xpos[body] + pos0, np.asarray(mat0).reshape(3, 3)
  if mode == 2:
    return com[body] + poscom0, np.asarray(mat0).reshape(3, 3)
  p = xpos[body] + xmat[body] @ pos
  if mode == 0:
    return p, xmat[body] @ quat_to_mat(quat)
  look = (xpos if mode == 3 else com)[target] - p
  z = -look / np.linalg.norm(look)
  x = np.cross([0.0, 0, 1], z)
  x = x / np.linalg.norm(x)
  return p, np.stack([x, np.cross(z, x), z], 1)


def pixel_dirs(fovy, H, W, dx=0.0, dy=0.0):
  """(H, W, 3) camera-frame directions; (dx, dy) shifts every pixel centre by that many pixels (edge probing)."""
  f = 0.5 * H / math.tan(math.radians(fovy) / 2)
  c, r = np.meshgrid(np.arange(W, dtype=np.float64) + dx, np.arange(H, dtype=np.float64) + dy)
  return np.stack([(c - (W - 1) / 2) / f, -(r - (H - 1) / 2) / f, -np.ones_like(c)], -1)


def _quadratic(a, b, c, ok_fn):
  """roots x of a x^2 + 2 b x + c = 0 that are >= 0 and pass ok_fn(x); nearest first.  Returns (t, valid)."""
  t = np.full(a.shape, np.inf)
  with np.errstate(all='ignore'):
    det = b*b - a*c
    good = (a >= MINVAL) & (det >= 0)
    sq = np.sqrt(np.where(good, det, 0))
    for x in ((-b - sq) / np.where(good, a, 1), (-b + sq) / np.where(good, a, 1)):
      m = good & (x >= 0) & ok_fn(x) & (x < t)
      t = np.where(m, x, t)
  return t


def ray_geom(gtype, size, lp, lv):
  """Nearest hit of the rays lp + t lv (lv: (N, 3)) with one primitive in its own frame.  Returns t (N,), inf where
  missed, and the outward unit normals (N, 3) at the hits."""
  N = lv.shape[0]
  t = np.full(N, np.inf)
  n = np.zeros((N, 3))
  s = np.asarray(size, dtype=np.float64)

  def take(tn, normal_fn):
    nonlocal t, n
    m = tn < t
    if m.any():
      t = np.where(m, tn, t)
      p = lp + np.where(np.isfinite(tn), tn, 0)[:, None] * lv
      n = np.where(m[:, None], normal_fn(p), n)

  def unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), MINVAL)

  with np.errstate(all='ignore'):
    if gtype == PLANE:
      x = -lp[2] / np.where(lv[:, 2] < -MINVAL, lv[:, 2], -1)
      px, py = lp[0] + x*lv[:, 0], lp[1] + x*lv[:, 1]
      ok = (lv[:, 2] < -MINVAL) & (x >= 0)
      if s[0] > 0:
        ok &= np.abs(px) <= s[0]
      if s[1] > 0:
        ok &= np.abs(py) <= s[1]
      take(np.where(ok, x, np.inf), lambda p: np.tile([0.0, 0, 1], (N, 1)))
    elif gtype == SPHERE:
      a = (lv*lv).sum(1); b = lv @ lp; c = lp @ lp - s[0]**2
      take(_quadratic(a, b, c, lambda x: True), unit)
    elif gtype == ELLIPSOID:
      q, w = lp / s, lv / s
      a = (w*w).sum(1); b = w @ q; c = q @ q - 1
      take(_quadratic(a, b, c, lambda x: True), lambda p: unit(p / (s*s)))
    elif gtype == CAPSULE:
      r, h = s[0], s[1]
      a = lv[:, 0]**2 + lv[:, 1]**2; b = lp[0]*lv[:, 0] + lp[1]*lv[:, 1]; c = lp[0]**2 + lp[1]**2 - r*r
      take(_quadratic(a, b, c, lambda x: np.abs(lp[2] + x*lv[:, 2]) <= h), lambda p: unit(p * [1, 1, 0]))
      for cz in (h, -h):
        q = lp - [0, 0, cz]
        a = (lv*lv).sum(1); b = lv @ q; c = q @ q - r*r
        side = (lambda x, cz=cz: (lp[2] + x*lv[:, 2] >= h) if cz > 0 else (lp[2] + x*lv[:, 2] <= -h))
        take(_quadratic(a, b, c, side), lambda p, cz=cz: unit(p - [0, 0, cz]))
    elif gtype == CYLINDER:
      r, h = s[0], s[1]
      a = lv[:, 0]**2 + lv[:, 1]**2; b = lp[0]*lv[:, 0] + lp[1]*lv[:, 1]; c = lp[0]**2 + lp[1]**2 - r*r
      take(_quadratic(a, b, c, lambda x: np.abs(lp[2] + x*lv[:, 2]) <= h), lambda p: unit(p * [1, 1, 0]))
      for sg in (-1.0, 1.0):
        okd = np.abs(lv[:, 2]) >= MINVAL
        x = (sg*h - lp[2]) / np.where(okd, lv[:, 2], 1)
        px, py = lp[0] + x*lv[:, 0], lp[1] + x*lv[:, 1]
        ok = okd & (x >= 0) & (px*px + py*py <= r*r)
        take(np.where(ok, x, np.inf), lambda p, sg=sg: np.tile([0.0, 0, sg], (N, 1)))
    elif gtype == BOX:
      for ax in range(3):
        a1, a2 = (ax + 1) % 3, (ax + 2) % 3
        okd = np.abs(lv[:, ax]) >= MINVAL
        for sg in (-1.0, 1.0):
          x = (sg*s[ax] - lp[ax]) / np.where(okd, lv[:, ax], 1)
          ok = okd & (x >= 0) & (np.abs(lp[a1] + x*lv[:, a1]) <= s[a1]) & (np.abs(lp[a2] + x*lv[:, a2]) <= s[a2])
          nv = np.zeros(3); nv[ax] = sg
          take(np.where(ok, x, np.inf), lambda p, nv=nv: np.tile(nv, (N, 1)))
  return t, n


def render(cam_pos, cam_mat, fovy, H, W, geom_type, geom_size, geom_xpos, geom_xmat, visible, color=None, near=0.0,
           far=np.inf, ambient=0.4, diffuse=0.6, background=(0, 0, 0), dx=0.0, dy=0.0):
  """One camera of one environment.  geom_size (ngeom, 3), geom_xpos (ngeom, 3), geom_xmat (ngeom, 3, 3), visible
  (ngeom) bool, color (ngeom, 3) in [0, 1].  Returns depth (H, W) float64 (far where missed), geom id (H, W) int (-1
  where missed), rgb (H, W, 3) uint8 (None without color)."""
  d = pixel_dirs(fovy, H, W, dx, dy).reshape(-1, 3)
  best = np.full(H*W, np.inf)
  gid = np.full(H*W, -1)
  shade = np.zeros(H*W)
  for g in range(len(geom_type)):
    if not visible[g] or int(geom_type[g]) not in DRAWN:
      continue
    Rg = np.asarray(geom_xmat[g]).reshape(3, 3)
    lp = Rg.T @ (cam_pos - geom_xpos[g])
    lv = d @ (Rg.T @ cam_mat).T
    t, n = ray_geom(int(geom_type[g]), geom_size[g], lp, lv)
    m = np.isfinite(t) & (t >= near) & (t <= far) & (t < best)
    best = np.where(m, t, best)
    gid = np.where(m, g, gid)
    cosang = -(n * lv).sum(1) / np.linalg.norm(d, axis=1)
    shade = np.where(m, ambient + diffuse * np.maximum(0, cosang), shade)
  hit = gid >= 0
  depth = np.where(hit, best, far).reshape(H, W)
  rgb = None
  if color is not None:
    col = np.where(hit[:, None], np.asarray(color)[np.maximum(gid, 0)] * shade[:, None], np.asarray(background, dtype=np.float64))
    rgb = np.floor(255 * np.clip(col, 0, 1) + 0.5).astype(np.uint8).reshape(H, W, 3)
  return depth, gid.reshape(H, W), rgb


def excluded(render_fn):
  """The edge rule: a pixel is excluded from comparison when the twin, probed at +-0.02 px in x and y, changes hit geom
  or changes depth by more than 1 %.  render_fn(dx, dy) -> (depth, gid, ...).  Returns a (H, W) bool mask."""
  d0, g0 = render_fn(0.0, 0.0)[:2]
  ex = np.zeros(d0.shape, dtype=bool)
  for dx, dy in ((0.02, 0), (-0.02, 0), (0, 0.02), (0, -0.02)):
    d, g = render_fn(dx, dy)[:2]
    with np.errstate(all='ignore'):
      rel = np.abs(d - d0) / np.maximum(np.abs(d0), MINVAL)
    ex |= (g != g0) | ((g0 >= 0) & (rel > 0.01))
  return ex


def effective_colors(geom_rgba, geom_matid, mat_rgba):
  """Base colour per geom: the material's rgba where the geom has one and its own rgba is the default grey."""
  col = np.array(geom_rgba, dtype=np.float64)[:, :3].copy()
  for g in range(len(col)):
    if geom_matid[g] >= 0 and tuple(geom_rgba[g]) == (0.5, 0.5, 0.5, 1.0):
      col[g] = mat_rgba[geom_matid[g]][:3]
  return col

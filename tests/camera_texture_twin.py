"""TEST INFRASTRUCTURE: a plain-numpy fp64 restatement of the camera's texture model (PARITY_ASSUMPTIONS.md, "Ray-cast
camera textures"), written from that specification and independent of the kernel.  Rays, poses and primitives come from
camera_twin.

A texture has W x H texels; nearest sampling is the ground truth: i = floor(frac(u) W), j = floor(frac(v) H).  Specs are
the complete dicts of camera.material_spec (type, builtin, rgb1, rgb2, mark, markrgb, width, height, texrepeat, texuniform).
"""
import numpy as np

import camera_twin as twin


def _wh(spec):
  W = int(spec['width'])
  return W, (int(spec['height']) or W) if spec['type'] == '2d' else W


def axis_class(i, W, mark):
  """0 mark, 1 first half, 2 second half, for texel column(s) i of a W-texel axis."""
  i = np.asarray(i)
  c = np.where(2*i < W, 1, 2)
  if mark == 'edge':
    c = np.where((i == 0) | (i == W - 1), 0, c)
  elif mark == 'cross':
    c = np.where(i == W // 2, 0, c)
  return c


def texel_index(u, W):
  u = np.asarray(u, dtype=np.float64)
  return np.clip(np.floor((u - np.floor(u)) * W).astype(np.int64), 0, W - 1)


def _smooth(p):
  return 3*p*p - 2*p*p*p


def class_color(spec, cu, cv, i, j):
  """Colour (..., 3) of texels with axis classes (cu, cv) and indices (i, j)."""
  W, H = _wh(spec)
  r1, r2, mk = (np.asarray(spec[k], dtype=np.float64) for k in ('rgb1', 'rgb2', 'markrgb'))
  cu, cv = np.asarray(cu), np.asarray(cv)
  if spec['builtin'] == 'flat':
    base = np.broadcast_to(r1, cu.shape + (3,))
  elif spec['builtin'] == 'checker':
    base = np.where((cu == cv)[..., None], r1, r2)
  elif spec['builtin'] == 'gradient':
    x, y = (2*np.asarray(i) + 1) / W - 1, (2*np.asarray(j) + 1) / H - 1
    p = np.minimum(1, np.sqrt(x*x + y*y))
    base = r1 + (r2 - r1) * _smooth(p)[..., None]
  else:
    raise ValueError(spec['builtin'])
  return np.where(((cu == 0) | (cv == 0))[..., None], mk, base)


def texel_color(spec, u, v):
  """Nearest sampling: colour (..., 3) at (u, v), and the class key 3 cu + cv of the texel."""
  W, H = _wh(spec)
  i, j = texel_index(u, W), texel_index(v, H)
  cu, cv = axis_class(i, W, spec['mark']), axis_class(j, H, spec['mark'])
  return class_color(spec, cu, cv, i, j), 3*cu + cv


def class_intervals(W, mark):
  """Per class, the intervals of [0, 1] its texels cover: unions of texel columns [i / W, (i + 1) / W)."""
  out = {0: [], 1: [], 2: []}
  cls = axis_class(np.arange(W), W, mark)
  for i in range(W):
    out[int(cls[i])].append((i / W, (i + 1) / W))
  return out


def class_boundaries(W, mark):
  """Positions in [0, 1) where the class changes between neighbouring texel columns (the wrap at 0 included)."""
  cls = axis_class(np.arange(W), W, mark)
  return [i / W for i in range(W) if cls[i] != cls[i - 1]]


def _antiderivative(x, a, b):
  """Integral over [0, x] of the 1-periodic indicator of [a, b)."""
  n = np.floor(x)
  return n*(b - a) + np.clip(x - n, a, b) - a


def class_shares(u, h, W, mark):
  """(..., 3): the exact share of [u - h, u + h] in each class (h > 0)."""
  u, h = np.asarray(u, dtype=np.float64), np.asarray(h, dtype=np.float64)
  out = np.zeros(np.broadcast(u, h).shape + (3,))
  for c, ivs in class_intervals(W, mark).items():
    for a, b in ivs:
      out[..., c] += (_antiderivative(u + h, a, b) - _antiderivative(u - h, a, b)) / (2*h)
  return out


def box_color(spec, u, v, hu, hv):
  """The mean of the nearest-sampled pattern over the box (u -+ hu, v -+ hv); the gradient is taken at the centre."""
  W, H = _wh(spec)
  wu, wv = class_shares(u, hu, W, spec['mark']), class_shares(v, hv, H, spec['mark'])
  i, j = texel_index(u, W), texel_index(v, H)
  out = np.zeros(np.shape(u) + (3,))
  for cu in range(3):
    for cv in range(3):
      out += (wu[..., cu] * wv[..., cv])[..., None] * class_color(spec, np.full(np.shape(u), cu), np.full(np.shape(u), cv), i, j)
  return out


def supersample(spec, u, v, hu, hv, N=64):
  """N x N midpoint rule of nearest sampling over the same box (scalars)."""
  k = (np.arange(N) + 0.5) / N
  uu, vv = np.meshgrid(u - hu + 2*hu*k, v - hv + 2*hv*k, indexing='ij')
  return texel_color(spec, uu, vv)[0].reshape(-1, 3).mean(0)


def boundaries_inside(lo, hi, W, mark):
  """How many class boundaries (all periods) lie in [lo, hi]."""
  n = 0
  for b in class_boundaries(W, mark):
    n += int(np.floor(hi - b) - np.ceil(lo - b) + 1)
  return max(n, 0)


def plane_uv(spec, size, px, py):
  """(u, v) and (du/dpx, dv/dpy) of points (px, py) of a plane geom's frame."""
  r0, r1 = spec['texrepeat']
  if spec['texuniform']:
    return px*r0, py*r1, r0, r1
  sx, sy = (size[0] if size[0] > 0 else 1.0), (size[1] if size[1] > 0 else 1.0)
  return r0*(px/(2*sx) + 0.5), r1*(py/(2*sy) + 0.5), r0/(2*sx), r1/(2*sy)


def cube_extents(gtype, size):
  s = np.asarray(size, dtype=np.float64)
  return {twin.BOX: s, twin.ELLIPSOID: s, twin.SPHERE: np.array([s[0]]*3), twin.CYLINDER: np.array([s[0], s[0], s[1]]),
          twin.CAPSULE: np.array([s[0], s[0], s[0] + s[1]])}[gtype]


def cube_uv(spec, gtype, size, q):
  """face (N,), u (N,), v (N,) of local points q (N, 3)."""
  q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
  if not spec['texuniform']:
    q = q / cube_extents(gtype, size)
  face = np.argmax(np.abs(q), axis=1)      # (the first maximum: the lowest axis on ties)
  n = np.arange(len(q))
  den = np.maximum(np.abs(q[n, face]), twin.MINVAL)
  a, b = q[n, (face + 1) % 3] / den, q[n, (face + 2) % 3] / den
  return face, spec['texrepeat'][0]*(a + 1)/2, spec['texrepeat'][1]*(b + 1)/2


def sky_color(spec, w):
  """Colour (N, 3) in [0, 1] for unit world directions w (N, 3)."""
  r1, r2 = np.asarray(spec['rgb1'], dtype=np.float64), np.asarray(spec['rgb2'], dtype=np.float64)
  if spec['builtin'] == 'flat':
    return np.broadcast_to(r1, (len(w), 3))
  p = (1 - w[:, 2]) / 2
  return r1 + (r2 - r1) * _smooth(p)[:, None]


def plane_footprint(cam_pos, cam_mat, f, d, gpos, Rg):
  """Half-widths (N, 2) in the plane's x and y of the pixels looking along camera-frame directions d (N, 3): 0.5 (|dp/dcol|
  + |dp/drow|) with p the plane-frame hit point, derived in WORLD terms: P = c + t w, w = Rcam d, t = n . (g - c) / (n . w)."""
  n = Rg[:, 2]
  w = d @ cam_mat.T
  nw = w @ n
  t = (n @ (gpos - cam_pos)) / nw
  half = np.zeros((len(d), 2))
  for k, sgn in ((0, 1.0), (1, -1.0)):      # d(dx)/d(col) = 1/f, d(dy)/d(row) = -1/f
    e = cam_mat[:, k] * (sgn / f)
    dP = t[:, None]*e - w * (t * (n @ e) / nw)[:, None]
    half += 0.5*np.abs(dP @ Rg[:, :2])
  return half


def render(cam_pos, cam_mat, fovy, H, W, geom_type, geom_size, geom_xpos, geom_xmat, visible, color, specs, sky=None,
           texture_filter='nearest', near=0.0, far=np.inf, ambient=0.4, diffuse=0.6, background=(0, 0, 0), dx=0.0, dy=0.0):
  """camera_twin.render with textures.  specs: per geom a complete material spec or None; sky: a spec or None.  Returns
  depth (H, W), gid (H, W), rgb (H, W, 3) uint8 and key (H, W) int -- the texel class pair and cube face under the pixel
  (-1 where untextured), whose change under a sub-pixel probe excludes the pixel."""
  import math
  f = 0.5 * H / math.tan(math.radians(fovy) / 2)
  d = twin.pixel_dirs(fovy, H, W, dx, dy).reshape(-1, 3)
  N = H*W
  best, gid = np.full(N, np.inf), np.full(N, -1)
  shade, tex, key = np.zeros(N), np.ones((N, 3)), np.full(N, -1)
  for g in range(len(geom_type)):
    gtype = int(geom_type[g])
    if not visible[g] or gtype not in twin.DRAWN:
      continue
    Rg = np.asarray(geom_xmat[g]).reshape(3, 3)
    lp = Rg.T @ (cam_pos - geom_xpos[g])
    lv = d @ (Rg.T @ cam_mat).T
    t, n = twin.ray_geom(gtype, geom_size[g], lp, lv)
    m = np.isfinite(t) & (t >= near) & (t <= far) & (t < best)
    if not m.any():
      continue
    best, gid = np.where(m, t, best), np.where(m, g, gid)
    cosang = -(n * lv).sum(1) / np.linalg.norm(d, axis=1)
    shade = np.where(m, ambient + diffuse * np.maximum(0, cosang), shade)
    spec = specs[g]
    tg, kg = np.ones((N, 3)), np.full(N, -1)
    if spec is not None:
      p = lp + np.where(m, t, 0)[:, None] * lv
      if spec['type'] == '2d' and gtype == twin.PLANE:
        u, v, su, sv = plane_uv(spec, geom_size[g], p[:, 0], p[:, 1])
        tg, kg = texel_color(spec, u, v)
        if texture_filter == 'box':
          with np.errstate(all='ignore'):
            half = plane_footprint(cam_pos, cam_mat, f, d, np.asarray(geom_xpos[g]), Rg)
            half = np.where(m[:, None], half, 1.0)
            tg = box_color(spec, u, v, abs(su)*half[:, 0], abs(sv)*half[:, 1])
          kg = np.full(N, -1)      # no discontinuities under the box filter
      elif spec['type'] == 'cube' and gtype != twin.PLANE:
        face, u, v = cube_uv(spec, gtype, geom_size[g], p)
        tg, kg = texel_color(spec, u, v)
        kg = kg + 9*face
    tex, key = np.where(m[:, None], tg, tex), np.where(m, kg, key)
  hit = gid >= 0
  depth = np.where(hit, best, far).reshape(H, W)
  base = np.asarray(color, dtype=np.float64)[np.maximum(gid, 0)] * tex * shade[:, None]
  if sky is not None:
    w = d @ cam_mat.T
    miss = sky_color(sky, w / np.linalg.norm(w, axis=1, keepdims=True))
  else:
    miss = np.broadcast_to(np.asarray(background, dtype=np.float64), (N, 3))
  col = np.where(hit[:, None], base, miss)
  rgb = np.floor(255 * np.clip(col, 0, 1) + 0.5).astype(np.uint8).reshape(H, W, 3)
  return depth, gid.reshape(H, W), rgb, key.reshape(H, W)


def excluded(render_fn):
  """camera_twin.excluded, extended: a change of the texture key (texel class pair, cube face) under the +-0.02 px probes
  excludes the pixel too.  render_fn(dx, dy) -> (depth, gid, rgb, key)."""
  ex = twin.excluded(render_fn)
  k0 = render_fn(0.0, 0.0)[3]
  for dx, dy in ((0.02, 0), (-0.02, 0), (0, 0.02), (0, -0.02)):
    ex |= render_fn(dx, dy)[3] != k0
  return ex

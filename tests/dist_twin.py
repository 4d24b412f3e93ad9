"""TEST INFRASTRUCTURE: the fp64 twin of the distance unit, written from the definition (PARITY_ASSUMPTIONS rows 61-66) and
not from GJK / EPA.  It knows nothing of cores: a geom is its support function, its projection and its surface function.

  dist = max over unit n of f(n),   f(n) = n.(cB - cA) - hA(n) - hB(-n)

  * apart: the constrained minimisation of |x - y| over x in A, y in B (scipy SLSQP from the centres, a convex problem),
    polished by alternating projections (closed-form projections; the ellipsoid's by a scalar Newton iteration).  The dual
    value f((y - x) / |y - x|) is a lower bound of the same distance: `gap` = |x - y| - f is the twin's own error bound.
  * overlapping (no x, y with |x - y| > 0 ...: f < 0 everywhere): the global maximisation of f over directions -- a dense
    Fibonacci sampling, the candidate axes a flat face or a straight edge make exact (face normals, axes, their cross
    products: the SAT axes for two boxes), and a local simplex refinement from the best few.  `second`: the best value
    among the refined optima whose direction differs from the winner's, for the uniqueness flag.  The DISTANCE of an
    overlap is independent of the solver; its WITNESS POINTS are not fully: given its own normal the twin, like the solver,
    moves geom2 out along it by the depth plus a gap and takes the closest points (by projections, not GJK).  What pins an
    overlap's witnesses independently are the invariants: both points on their surfaces, |to - from| = |dist|.
"""
import numpy as np

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = 0, 2, 3, 4, 5, 6
RADIUS = {SPHERE: True, CAPSULE: True}      # the types with a rounding radius (size[0]): "shallow" overlap exists for them


def quat_to_mat(q):
  w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
  return np.array([[1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y)],
                   [2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x)],
                   [2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)]])


class Geom:
  def __init__(self, type_, size, pos, mat):
    self.type, self.size = int(type_), np.asarray(size, dtype=np.float64).reshape(3)
    self.pos, self.mat = np.asarray(pos, dtype=np.float64).reshape(3), np.asarray(mat, dtype=np.float64).reshape(3, 3)

  # -- support: local directions (N, 3) -> local points (N, 3)
  def support_local(self, d):
    d = np.atleast_2d(d)
    s, t = self.size, self.type
    nrm = np.linalg.norm(d, axis=1, keepdims=True)
    u = d / np.where(nrm > 0, nrm, 1)
    sgn = lambda v: np.where(v >= 0, 1.0, -1.0)
    if t == SPHERE:
      return s[0]*u
    if t == CAPSULE:
      p = s[0]*u
      p[:, 2] += s[1]*sgn(u[:, 2])
      return p
    if t == ELLIPSOID:
      a = s*s*u
      return a / np.sqrt(np.sum(a*u, axis=1, keepdims=True))
    if t == CYLINDER:
      rho = np.linalg.norm(u[:, :2], axis=1, keepdims=True)
      p = np.zeros_like(u)
      p[:, :2] = s[0]*u[:, :2] / np.where(rho > 0, rho, 1)
      p[:, 2] = s[1]*sgn(u[:, 2])
      return p
    if t == BOX:
      return s*sgn(u)
    raise ValueError('no support function for geom type %d' % t)

  def support(self, n):
    """World support points along world directions n (N, 3)."""
    return self.pos + self.support_local(np.atleast_2d(n) @ self.mat) @ self.mat.T

  def h(self, n):
    """Support function about the centre: max over the geom of n.(p - pos), n (N, 3) unit."""
    n = np.atleast_2d(n)
    return np.sum(self.support_local(n @ self.mat) * (n @ self.mat), axis=1)

  # -- projection of a world point onto the (closed) set
  def project(self, p):
    q = self.mat.T @ (np.asarray(p, dtype=np.float64) - self.pos)
    s, t = self.size, self.type
    if t == SPHERE:
      r = np.linalg.norm(q)
      q = q if r <= s[0] else q*(s[0]/r)
    elif t == CAPSULE:
      c = np.array([0, 0, np.clip(q[2], -s[1], s[1])])
      r = np.linalg.norm(q - c)
      q = q if r <= s[0] else c + (q - c)*(s[0]/r)
    elif t == ELLIPSOID:
      if np.sum((q/s)**2) > 1:
        lam = 0.0      # q_i s_i^2 / (s_i^2 + lam) on the surface: g(lam) = sum (s_i q_i / (s_i^2 + lam))^2 - 1, decreasing, convex
        for _ in range(100):
          den = s*s + lam
          g = np.sum((s*q/den)**2) - 1
          dg = -2*np.sum((s*q)**2/den**3)
          step = g/dg
          lam -= step
          if abs(step) <= 1e-16*max(1.0, abs(lam)):
            break
        q = q*s*s/(s*s + lam)
    elif t == CYLINDER:
      r = np.hypot(q[0], q[1])
      k = 1.0 if r <= s[0] else s[0]/r
      q = np.array([q[0]*k, q[1]*k, np.clip(q[2], -s[1], s[1])])
    elif t == BOX:
      q = np.clip(q, -s, s)
    else:
      raise ValueError('no projection for geom type %d' % t)
    return self.pos + self.mat @ q

  def surface(self, p):
    """Signed distance-like surface function of a world point: 0 on the surface (exact distance for all but the ellipsoid,
    whose value is the distance to the projection outside and a first-order estimate inside)."""
    if self.type == PLANE:
      return float(self.mat[:, 2] @ (np.asarray(p) - self.pos))
    q = self.mat.T @ (np.asarray(p, dtype=np.float64) - self.pos)
    s, t = self.size, self.type
    if t == SPHERE:
      return np.linalg.norm(q) - s[0]
    if t == CAPSULE:
      return np.linalg.norm(q - [0, 0, np.clip(q[2], -s[1], s[1])]) - s[0]
    if t == ELLIPSOID:
      k = np.sqrt(np.sum((q/s)**2))
      if k > 1:
        return np.linalg.norm(np.asarray(p) - self.project(p))
      return (k - 1)*k / max(np.linalg.norm(q/(s*s)), 1e-300) if k > 0 else -s.min()
    if t == CYLINDER:
      e = np.array([np.hypot(q[0], q[1]) - s[0], abs(q[2]) - s[1]])
    else:
      e = np.abs(q) - s
    return np.linalg.norm(np.maximum(e, 0)) + min(e.max(), 0.0)


def f_dir(A, B, n):
  n = np.atleast_2d(n)
  return n @ (B.pos - A.pos) - A.h(n) - B.h(-n)


_FIB = None


def _fibonacci(N=20000):
  global _FIB
  if _FIB is None or len(_FIB) != N:
    i = np.arange(N) + 0.5
    z = 1 - 2*i/N
    phi = np.pi*(1 + 5**0.5)*i
    r = np.sqrt(1 - z*z)
    _FIB = np.stack([r*np.cos(phi), r*np.sin(phi), z], 1)
  return _FIB


def _axes(g):
  if g.type == BOX:
    return [g.mat[:, k] for k in range(3)]
  if g.type in (CAPSULE, CYLINDER):
    return [g.mat[:, 2]]
  return []


def _refine(A, B, n0):
  from scipy import optimize
  n0 = n0/np.linalg.norm(n0)
  t1 = np.cross(n0, [1.0, 0, 0] if abs(n0[0]) < 0.9 else [0, 1.0, 0])
  t1 /= np.linalg.norm(t1)
  t2 = np.cross(n0, t1)
  def neg(u):
    n = n0 + u[0]*t1 + u[1]*t2
    return -float(f_dir(A, B, n/np.linalg.norm(n))[0])
  best_u, best_f = np.zeros(2), neg(np.zeros(2))
  for scale in (0.05, 1e-3, 1e-5):      # restarts of the simplex at shrinking sizes: it stalls on the kinks of a box
    r = optimize.minimize(neg, best_u, method='Nelder-Mead',
                          options=dict(xatol=1e-15, fatol=1e-17, maxiter=600, initial_simplex=best_u + scale*np.array([[0, 0], [1, 0], [0, 1.0]])))
    if r.fun < best_f:
      best_u, best_f = r.x, r.fun
  n = n0 + best_u[0]*t1 + best_u[1]*t2
  return n/np.linalg.norm(n), -best_f


def plane_distance(P, G):
  n = P.mat[:, 2]
  p = G.support(-n[None])[0]
  return float(n @ (p - P.pos)), p, n


def distance(A, B, nstart=4):
  """dict(dist, fromto (6,), gap, second): the definition's value for two geoms (a plane on either side allowed)."""
  if A.type == PLANE and B.type == PLANE:
    raise ValueError('plane-plane has no distance')
  if A.type == PLANE or B.type == PLANE:
    P, G = (A, B) if A.type == PLANE else (B, A)
    d, p, n = plane_distance(P, G)
    on_plane = p - d*n
    ft = np.concatenate([on_plane, p]) if A.type == PLANE else np.concatenate([p, on_plane])
    return dict(dist=d, fromto=ft, gap=0.0, second=-np.inf)
  # apart? alternating projections from the centres decide (they converge to a common point when the sets meet)
  x, y = _closest(A, B)
  d = np.linalg.norm(y - x)
  scale = 1.0
  if d > 1e-9:
    n = (y - x)/d
    lower = float(f_dir(A, B, n)[0])
    if lower > 0:
      return dict(dist=d, fromto=np.concatenate([x, y]), gap=d - lower, second=-np.inf)
  # overlapping: global maximisation over directions
  dirs = _fibonacci()
  vals = f_dir(A, B, dirs)
  order = np.argsort(-vals)
  starts = []
  for i in order:      # the best few samples that are not neighbours of one another
    if all(dirs[i] @ s < np.cos(0.15) for s in starts):
      starts.append(dirs[i])
    if len(starts) == nstart:
      break
  cands = []
  ax = _axes(A) + _axes(B)
  for a in _axes(A):
    for b in _axes(B):
      c = np.cross(a, b)
      if np.linalg.norm(c) > 1e-9:
        ax.append(c/np.linalg.norm(c))
  for a in ax:
    cands += [a, -a]
  exact = [(float(f_dir(A, B, c)[0]), c) for c in cands]
  refined = [(_refine(A, B, s)[::-1]) for s in starts]
  if exact:      # the best exact axis, refined too (a no-op where it is the optimum)
    fb, cb = max(exact, key=lambda t: t[0])
    refined.append(_refine(A, B, cb)[::-1])
    refined.append((fb, cb))
  fbest, nbest = max(refined, key=lambda t: t[0])
  others = [f for f, n in refined if n @ nbest < np.cos(0.05)]
  second = max(others) if others else -np.inf
  # witness points: move B out along n by the depth (they touch) and find the common point
  depth = -fbest
  Bs = Geom(B.type, B.size, B.pos + (depth + 1e-3*scale)*nbest, B.mat)
  xs, ys = _closest(A, Bs)
  frm = xs
  to = frm + fbest*nbest
  return dict(dist=fbest, fromto=np.concatenate([frm, to]), gap=0.0, second=second)


def _closest(A, B, iters=4000):
  """Closest points of two convex sets: SLSQP on (x, y) from the centres, then alternating projections to a fixed point."""
  from scipy import optimize
  def cons(g, sl):
    s, t = g.size, g.type
    loc = lambda z: g.mat.T @ (z[sl] - g.pos)
    if t == SPHERE:
      return [lambda z: s[0]**2 - np.sum(loc(z)**2)]
    if t == CAPSULE:
      def c(z):
        q = loc(z)
        return s[0]**2 - np.sum((q - [0, 0, np.clip(q[2], -s[1], s[1])])**2)
      return [c]
    if t == ELLIPSOID:
      return [lambda z: 1 - np.sum((loc(z)/s)**2)]
    if t == CYLINDER:
      return [lambda z: s[0]**2 - np.sum(loc(z)[:2]**2), lambda z: s[1] - loc(z)[2], lambda z: s[1] + loc(z)[2]]
    return [lambda z, k=k, sg=sg: s[k] - sg*loc(z)[k] for k in range(3) for sg in (1, -1)]
  z0 = np.concatenate([A.pos, B.pos])
  if np.linalg.norm(A.pos - B.pos) > 1e-12:
    r = optimize.minimize(lambda z: np.sum((z[:3] - z[3:])**2), z0, jac=lambda z: 2*np.concatenate([z[:3] - z[3:], z[3:] - z[:3]]),
                          method='SLSQP', constraints=[dict(type='ineq', fun=c) for c in cons(A, slice(0, 3)) + cons(B, slice(3, 6))],
                          options=dict(ftol=1e-16, maxiter=200))
    z0 = r.x
  x, y = A.project(z0[:3]), B.project(z0[3:])
  for _ in range(iters):
    xn = A.project(y)
    yn = B.project(xn)
    moved = max(np.max(np.abs(xn - x)), np.max(np.abs(yn - y)))
    x, y = xn, yn
    if moved <= 1e-16:
      break
  return x, y


# ---- closed forms the twin's accuracy is measured against ---------------------------------------------------------
def closed_form(A, B):
  """The exact distance where a closed form exists for the pair as posed, else None: sphere-sphere, sphere-capsule,
  capsule-capsule, sphere-box, and box-box by SAT while overlapping."""
  ta, tb = A.type, B.type
  if ta > tb:
    return closed_form(B, A)
  seg = lambda g: (g.pos - g.size[1]*g.mat[:, 2], g.pos + g.size[1]*g.mat[:, 2])
  if (ta, tb) == (SPHERE, SPHERE):
    return np.linalg.norm(A.pos - B.pos) - A.size[0] - B.size[0]
  if (ta, tb) == (SPHERE, CAPSULE):
    p, q = seg(B)
    t = np.clip((A.pos - p) @ (q - p)/((q - p) @ (q - p)), 0, 1)
    return np.linalg.norm(A.pos - (p + t*(q - p))) - A.size[0] - B.size[0]
  if (ta, tb) == (CAPSULE, CAPSULE):
    return _seg_seg(*seg(A), *seg(B)) - A.size[0] - B.size[0]
  if (ta, tb) == (SPHERE, BOX):
    q = B.mat.T @ (A.pos - B.pos)
    e = np.abs(q) - B.size
    return np.linalg.norm(np.maximum(e, 0)) + min(e.max(), 0.0) - A.size[0]
  if (ta, tb) == (BOX, BOX):
    axes = [A.mat[:, k] for k in range(3)] + [B.mat[:, k] for k in range(3)]
    for i in range(3):
      for j in range(3):
        c = np.cross(A.mat[:, i], B.mat[:, j])
        if np.linalg.norm(c) > 1e-9:
          axes.append(c/np.linalg.norm(c))
    n = np.array(axes + [-a for a in axes])
    best = float(np.max(f_dir(A, B, n)))
    return best if best < 0 else None      # apart, the largest SAT separation is not the Euclidean distance
  return None


def _seg_seg(p1, q1, p2, q2):
  """Distance of two segments (Ericson, Real-Time Collision Detection 5.1.9)."""
  d1, d2, r = q1 - p1, q2 - p2, p1 - p2
  a, e, f = d1 @ d1, d2 @ d2, d2 @ r
  c, b = d1 @ r, d1 @ d2
  den = a*e - b*b
  s = np.clip((b*f - c*e)/den, 0, 1) if den > 1e-300 else 0.0
  t = (b*s + f)/e
  if t < 0:
    t, s = 0.0, np.clip(-c/a, 0, 1)
  elif t > 1:
    t, s = 1.0, np.clip((b - c)/a, 0, 1)
  return np.linalg.norm(p1 + s*d1 - p2 - t*d2)

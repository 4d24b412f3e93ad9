"""TEST INFRASTRUCTURE: the scenes, poses, oracle references, matcher and edge rule of the contact-level tests (CPU tier:
tests/test_contacts_cpu.py on the host build; GPU tier: tests/test_gpu_contacts.py).  The contact list of one `forward` is
compared with the fp64 oracle's contact by contact and IN ORDER: geoms, dist, pos, normal and tangents."""
import functools

import numpy as np

from dm_control_amd import mjcf_compiler as mc
from oracle.oracle import OracleModel, OraclePhysics
from ray_cases import EDGE_CAP, TOL_F64, TOL_F32_ONE_STEP

MARGIN = 0.02
NPOSE = 64
QUANTITIES = ('dist', 'pos', 'normal', 'frame')
WARN_CONTACTFULL, WARN_COLLISION = 1, 8      # include/dmc_model_layout.h

# no two equal semi-axes anywhere: a swapped axis shows
SIZES = {'sphere': '.11', 'capsule': '.07 .16', 'box': '.12 .09 .15', 'cylinder': '.1 .13', 'ellipsoid': '.14 .08 .11'}
RBOUND = {'sphere': .11, 'capsule': .23, 'box': float(np.linalg.norm([.12, .09, .15])), 'cylinder': float(np.hypot(.1, .13)),
          'ellipsoid': .14}
PAIRS = ([('plane', t) for t in ('sphere', 'capsule', 'box', 'cylinder', 'ellipsoid')] +
         [('sphere', t) for t in ('sphere', 'capsule', 'box', 'cylinder', 'ellipsoid')] +
         [('capsule', t) for t in ('capsule', 'box', 'cylinder', 'ellipsoid')] + [('box', 'box'), ('ellipsoid', 'ellipsoid')])
# tested as the cylinder's enclosing capsule: never a contact, DMC_WARN_COLLISION where the oracle counts one
GUARDED = [('cylinder', 'cylinder'), ('box', 'cylinder')]
REFUSED = ('ellipsoid', 'box')      # no narrow phase and no guard: the batch is refused at create time


# the largest centre distance the sampler draws, as a share of the bounding spheres' (long bodies rarely touch near it)
REACH = {('sphere', 'capsule'): .85, ('capsule', 'capsule'): .62, ('capsule', 'box'): .8, ('capsule', 'cylinder'): .62,
         ('capsule', 'ellipsoid'): .8}


def pair_class(t1, t2):
  return 'ellipsoid' if 'ellipsoid' in (t1, t2) else 'analytic'


def pair_xml(t1, t2):
  """Gravity off; geom `a` is the world plane or sits on free body A, geom `b` on free body B."""
  a = ('<geom name="a" type="plane" size="3 3 .1" margin="%g"/>' % MARGIN) if t1 == 'plane' else \
      '<body name="A"><freejoint/><geom name="a" type="%s" size="%s" margin="%g"/></body>' % (t1, SIZES[t1], MARGIN)
  return ('<mujoco><option gravity="0 0 0"/><worldbody>%s<body name="B" pos="0 0 1"><freejoint/>'
          '<geom name="b" type="%s" size="%s" margin="%g"/></body></worldbody></mujoco>') % (a, t2, SIZES[t2], MARGIN)


@functools.lru_cache(maxsize=None)
def pair_model(t1, t2):
  return mc.compile_xml(pair_xml(t1, t2))


def _quat(rs):
  q = rs.normal(size=4)
  return q/np.linalg.norm(q)


def quat_mat(q):
  w, x, y, z = q
  return np.array([[1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y)],
                   [2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x)],
                   [2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)]])


def sampled_poses(t1, t2, n=NPOSE):
  """n seeded poses of the pair scene: random orientations of both bodies, centre distances from deep overlap to just
  past the bounding spheres, so that most poses bear contacts of either sign of dist."""
  rs = np.random.RandomState(5 + 7*(PAIRS + GUARDED).index((t1, t2)))
  out = []
  for _ in range(n):
    qb = _quat(rs)
    if t1 == 'plane':
      p = np.array([rs.uniform(-1, 1), rs.uniform(-1, 1), rs.uniform(0.3*min(RBOUND[t2], .07), RBOUND[t2] + MARGIN)])
      out.append(np.concatenate([p, qb]))
    else:
      d = rs.normal(size=3)
      d /= np.linalg.norm(d)
      r = rs.uniform(0.35, REACH.get((t1, t2), 1.0))*(RBOUND[t1] + RBOUND[t2] + MARGIN)
      out.append(np.concatenate([rs.uniform(-.5, .5, 3), _quat(rs), np.zeros(3), qb]))
      out[-1][7:10] = out[-1][:3] + d*r
  return np.array(out)


_ID = (1., 0, 0, 0)
_Z2X = (np.sqrt(.5), 0, np.sqrt(.5), 0)      # the body's z axis along world x
_EPS = 0.005                                  # the directed poses hover this far apart: inside the margin, dist > 0


def _two(pa, qa, pb, qb):
  return np.concatenate([pa, qa, pb, qb]).astype(np.float64)


def _one(pb, qb):
  return np.concatenate([pb, qb]).astype(np.float64)


def _shared_parallel():
  """Parallel capsules in a shared random orientation: B beside A (0.13 across the axis) and 0.05 along it."""
  rs = np.random.RandomState(11)
  q = _quat(rs)
  R = quat_mat(q)
  pa = rs.uniform(-.5, .5, 3)
  return _two(pa, q, pa + 0.13*R[:, 0] + 0.05*R[:, 2], q)


def _rot(axis, angle):
  return np.r_[np.cos(angle/2), np.sin(angle/2)*np.asarray(axis, float)]


def directed_poses():
  """The branches a random pose never meets: [(name, t1, t2, qpos, contacts the oracle must count there)]."""
  s = .11 + _EPS      # sphere radius + hover
  return [
      ('parallel capsules', 'capsule', 'capsule', _two([0, 0, 0], _ID, [.13, 0, .05], _ID), 2),
      ('parallel capsules, shared random orientation', 'capsule', 'capsule', _shared_parallel(), 2),
      ('capsule flat on the plane', 'plane', 'capsule', _one([.2, -.1, .07 + _EPS], _Z2X), 2),
      ('box flat on the plane', 'plane', 'box', _one([.3, .1, .15 + _EPS], _ID), 4),
      ('box flat on a box', 'box', 'box', _two([0, 0, 0], _ID, [.03, .02, .3 + _EPS], _ID), 4),
      ('box edge across a box edge', 'box', 'box',
       _two([0, 0, 0], _rot([0, 1, 0], np.pi/4), [0, 0, (.12 + .15 + .09 + .15)/np.sqrt(2) + _EPS], _rot([1, 0, 0], np.pi/4)), 1),
      ('cylinder flat on the plane', 'plane', 'cylinder', _one([0, .2, .13 + _EPS], _ID), 3),
      ('cylinder on its rim on the plane', 'plane', 'cylinder',
       _one([0, .2, .13*np.cos(.4) + .1*np.sin(.4) + _EPS], _rot([1, 0, 0], .4)), 1),
      ('cylinder on its side on the plane', 'plane', 'cylinder', _one([.1, 0, .1 + _EPS], _Z2X), 2),
      ('sphere at a box face', 'sphere', 'box', _two([.02, .01, .15 + s], _ID, [0, 0, 0], _ID), 1),
      ('sphere at a box edge', 'sphere', 'box', _two([.12 + s/np.sqrt(2), .01, .15 + s/np.sqrt(2)], _ID, [0, 0, 0], _ID), 1),
      ('sphere at a box corner', 'sphere', 'box',
       _two([.12 + s/np.sqrt(3), .09 + s/np.sqrt(3), .15 + s/np.sqrt(3)], _ID, [0, 0, 0], _ID), 1),
      ('concentric spheres', 'sphere', 'sphere', _two([.1, .2, .3], _ID, [.1, .2, .3], _ID), 1),
  ]


def pair_poses(t1, t2):
  """(qpos (n, nq), names): the sampled poses of the pair scene followed by its directed ones."""
  q = [sampled_poses(t1, t2)]
  names = [None]*NPOSE
  for name, a, b, pose, _ in directed_poses():
    if (a, b) == (t1, t2):
      q.append(pose[None])
      names.append(name)
  return np.concatenate(q, 0), names


# ---- the heap: more candidate pairs than lanes, more contacts than a small cap ------------------------------------------------
HEAP_TYPES = ['sphere', 'capsule', 'box', 'capsule', 'sphere', 'box', 'capsule', 'box', 'sphere', 'capsule']
HEAP_NPAIR = 75      # 45 among the free bodies + 10 x (plane, pillar, post)
HEAP_NSTATE = 6
HEAP_SEEDS = (0, 1, 2, 4, 5, 8)      # 26 .. 44 contacts each (asserted from the oracle)
HEAP_NCONMAX = 48    # above every state's count; HEAP_SMALL_CAP: below every state's
HEAP_SMALL_CAP = 24


@functools.lru_cache(maxsize=None)
def heap_model():
  bodies = ''.join('<body name="b%d" pos="%g 0 1"><freejoint/><geom name="g%d" type="%s" size="%s" margin="%g"/></body>'
                   % (i, i, i, t, SIZES[t], MARGIN) for i, t in enumerate(HEAP_TYPES))
  return mc.compile_xml(
      '<mujoco><worldbody><geom name="floor" type="plane" size="3 3 .1" margin="%g"/>'
      '<geom name="pillar" type="box" size=".05 .05 .3" pos="0 0 .3" margin="%g"/>'
      '<geom name="post" type="capsule" size=".04 .3" pos=".15 .1 .3" margin="%g"/>%s</worldbody></mujoco>'
      % (MARGIN, MARGIN, MARGIN, bodies))


def heap_states():
  """(HEAP_NSTATE, nq): ten bodies thrown into a 0.5 m square at random heights and orientations."""
  m = heap_model()
  out = np.zeros((HEAP_NSTATE, m.nq))
  for k, seed in enumerate(HEAP_SEEDS):
    rs = np.random.RandomState(seed)
    for i in range(len(HEAP_TYPES)):
      out[k, 7*i:7*i + 3] = [rs.uniform(-.25, .25), rs.uniform(-.25, .25), rs.uniform(.08, .45)]
      out[k, 7*i + 3:7*i + 7] = _quat(rs)
  return out


# ---- the caps of the suite models ----------------------------------------------------------------------------------------------
# (asset, nconmax asked for: the production caps of suite/common.py) -> (nconmax, njmax) of the parent commit
SUITE_CAPS = {'acrobot': (0, 8, 32), 'ball_in_cup': (0, 16, 65), 'cartpole': (0, 12, 49), 'cheetah': (0, 16, 70),
              'cmu_2019_position_floor': (48, 48, 200), 'finger': (0, 16, 51), 'fish': (0, 16, 64), 'hopper': (0, 16, 68),
              'humanoid': (24, 24, 117), 'humanoid_CMU': (96, 96, 440), 'lqr': (0, 1, 1), 'manipulator': (24, 24, 80),
              'pendulum': (0, 7, 28), 'point_mass': (0, 6, 26), 'quadruped': (0, 16, 180), 'reacher': (0, 16, 65),
              'soccer_2v2_boxhead': (24, 24, 148), 'stacker': (48, 48, 152), 'swimmer': (0, 15, 60),
              'testing_humanoid_pgs': (0, 16, 81), 'walker': (0, 14, 62)}


# ---- the oracle's side ----------------------------------------------------------------------------------------------------------
class Ref:
  """The oracle's contact list of one pose."""

  def __init__(self, o):
    cs = [o.contact(i) for i in range(o.ncon)]
    self.ncon = o.ncon
    self.pairs = [(c['geom1'], c['geom2']) for c in cs]
    self.dist = np.array([c['dist'] for c in cs])
    self.pos = np.array([c['pos'] for c in cs]).reshape(-1, 3)
    self.frame = np.array([c['frame'] for c in cs]).reshape(-1, 3, 3)
    self.warning = np.array(o.warning)


def oracle_ref(model, q, edit=None):
  """`model`: a compiled model or an OracleModel; edit(oracle_model) rewrites model fields first (per-env geoms)."""
  o = OraclePhysics(model)
  if edit is not None:
    edit(o.model)
  o.qpos[:] = q
  o.forward()
  return Ref(o)


def is_edge(om, q, ref, move=None, edit=None):
  """The edge rule, from the oracle alone: the pose is an edge if the oracle's list of contact pairs differs between
  qpos, float32(qpos) and qpos with the coordinates `move` (body B's position) displaced by +-2e-6 along the first
  contact's normal -- the line of centres where there is no contact, a seeded sign pattern on every coordinate where
  `move` is None (scenes of many bodies) -- or if some contact has | dist - margin | < 1e-5."""
  if ref.ncon and np.abs(ref.dist - MARGIN).min() < 1e-5:
    return True
  variants = [np.asarray(q, np.float32).astype(np.float64)]
  for sign in (1, -1):
    v = np.array(q, dtype=np.float64)
    if move is None:
      v += sign*2e-6*np.where(np.random.RandomState(1).rand(v.size) < 0.5, -1.0, 1.0)
    else:
      if ref.ncon:
        n = ref.frame[0, 0]
      else:
        n = v[move] - v[:3] if move.start else np.array([0, 0, 1.0])
        n = n/max(np.linalg.norm(n), 1e-12)
      v[move] += sign*2e-6*n
    variants.append(v)
  return any(oracle_ref(om, v, edit).pairs != ref.pairs for v in variants)


class Case:
  """One batch of poses of one model with the oracle's references (computed once, shared by the tests, never changed)."""

  def __init__(self, name, model, qpos, cls, names=None, move=None, edits=None):
    self.name, self.model, self.qpos, self.cls, self.move = name, model, np.asarray(qpos, np.float64), cls, move
    self.names = names or [None]*len(self.qpos)
    self.edits = edits
    self.boxes = {g for g in range(len(model.geom_type)) if int(model.geom_type[g]) == 6}
    om = OracleModel(model)
    self.refs = [oracle_ref(model if edits else om, q, edits[e] if edits else None) for e, q in enumerate(self.qpos)]
    self._om, self._edge = om, None

  @property
  def edge(self):
    """(n,) bool: the poses the edge rule leaves out IN FP32 ONLY."""
    if self._edge is None:
      self._edge = np.array([is_edge(self.model if self.edits else self._om, q, r, self.move, self.edits[e] if self.edits else None)
                             for e, (q, r) in enumerate(zip(self.qpos, self.refs))])
    return self._edge


@functools.lru_cache(maxsize=None)
def pair_case(t1, t2):
  q, names = pair_poses(t1, t2)
  return Case('%s-%s' % (t1, t2), pair_model(t1, t2), q, pair_class(t1, t2), names,
              move=slice(0, 3) if t1 == 'plane' else slice(7, 10))


@functools.lru_cache(maxsize=None)
def heap_case(B=HEAP_NSTATE):
  """B environments over the six states (environment e holds state e % 6)."""
  return Case('heap', heap_model(), heap_states()[np.arange(B) % HEAP_NSTATE], 'analytic')


# ---- the matcher ----------------------------------------------------------------------------------------------------------------
class Listing:
  """One environment's contact list as a kernel published it."""

  def __init__(self, ncon, geom1, geom2, dist, pos, frame, warning):
    self.ncon = int(ncon)
    n = self.ncon
    self.pairs = [(int(a), int(b)) for a, b in zip(np.ravel(geom1)[:n], np.ravel(geom2)[:n])]
    self.dist = np.ravel(dist)[:n].astype(np.float64)
    self.pos = np.ravel(pos)[:3*n].reshape(n, 3).astype(np.float64)
    self.frame = np.ravel(frame)[:9*n].reshape(n, 3, 3).astype(np.float64)
    self.warning = np.ravel(warning)


def listings(get, B):
  """[Listing] of a batch from get(name) -> (B, rows)."""
  f = {n: get(n) for n in ('ncon', 'contact_geom1', 'contact_geom2', 'contact_dist', 'contact_pos', 'contact_frame', 'warning')}
  return [Listing(f['ncon'][e, 0], f['contact_geom1'][e], f['contact_geom2'][e], f['contact_dist'][e], f['contact_pos'][e],
                  f['contact_frame'][e], f['warning'][e]) for e in range(B)]


TIE = 1e-6      # two depths of one pair's contacts closer than this are a tie: equal in exact arithmetic, ordered by rounding


def _tied_runs(ref, n, boxes):
  """Runs [a, b) of one box-box pair's contacts in the oracle's list of which two have the same depth and which begin
  among its first n (a cap may cut the last one: b > n)."""
  out, a = [], 0
  while a < n:
    b = a + 1
    while b < ref.ncon and ref.pairs[b] == ref.pairs[a]:
      b += 1
    if b - a > 1 and ref.pairs[a][0] in boxes and ref.pairs[a][1] in boxes and (np.diff(np.sort(ref.dist[a:b])) < TIE).any():
      out.append((a, b))
    a = b
  return out


def match(got, ref, cap=None, what='', prec=64, boxes=()):
  """Worst error of each quantity of one pose; the ordered list of (geom1, geom2) must EQUAL the oracle's (with `cap`:
  the oracle's first `cap`) and the contacts are compared one by one in that order.  Where an oracle normal has |n_y|
  within 1e-4 of 0.5, make_frame picks its seed axis and fp32 may pick the other: that pose's tangents are left out (its
  normals are not).

  fp32 only, box against box (`boxes`: the model's box geoms): the contacts of the pair come out of comparisons between
  depths (which four vertices of the clipped polygon of up to eight are kept, and which comes first).  Where the oracle has two of them at the same
  depth -- parallel faces: the planar boxes of stacker, the upright heads of the soccer players -- rounding decides the
  comparison and fp32 keeps another, equally deep choice.  Of such a run the depths are compared as a set and the normals
  one by one, the positions and tangents not (a run that the cap cuts: the normals alone).  Every other contact, and
  all of fp64, is compared in full and in order."""
  n = ref.ncon if cap is None else min(ref.ncon, cap)
  assert got.pairs == ref.pairs[:n], '%s: contact list %s, the oracle has %s' % (what, got.pairs, ref.pairs[:n])
  err = dict.fromkeys(QUANTITIES, 0.0)
  if n:
    gd, rd, full, deep = got.dist.copy(), ref.dist[:n].copy(), np.ones(n, bool), np.ones(n, bool)
    for a, b in (_tied_runs(ref, n, boxes) if prec == 32 else []):
      full[a:b] = False
      if b <= n:
        gd[a:b], rd[a:b] = np.sort(gd[a:b]), np.sort(rd[a:b])
      else:
        deep[a:n] = False
    err['dist'] = float(np.abs(gd - rd)[deep].max()) if deep.any() else 0.0
    err['pos'] = float(np.abs(got.pos - ref.pos[:n])[full].max()) if full.any() else 0.0
    err['normal'] = float(np.abs(got.frame[:, 0] - ref.frame[:n, 0]).max())
    seed_switch = (np.abs(np.abs(ref.frame[:n, 0, 1]) - 0.5) < 1e-4).any()
    err['frame'] = err['normal'] if seed_switch or not full.any() else max(err['normal'], float(np.abs(got.frame - ref.frame[:n])[full].max()))
  return err


def worst(errs):
  return {k: max([e[k] for e in errs] or [0.0]) for k in QUANTITIES}


def check_case(case, got, prec, cap=None, exclude_edges=True):
  """Matches every pose of a case (fp32: but the edge poses); returns (worst errors, share of poses left out).  The
  warnings must be the oracle's too: DMC_WARN_COLLISION where it counts one, CONTACTFULL exactly where a cap cuts."""
  errs = []
  skip = case.edge if (prec == 32 and exclude_edges) else np.zeros(len(case.qpos), bool)
  for e, (g, r) in enumerate(zip(got, case.refs)):
    if skip[e]:
      continue
    what = '%s pose %d%s' % (case.name, e, ' (%s)' % case.names[e] if case.names[e] else '')
    errs.append(match(g, r, cap, what, prec, case.boxes))
    assert int(g.warning[WARN_COLLISION] > 0) == int(r.warning[WARN_COLLISION] > 0), what
    assert int(g.warning[WARN_CONTACTFULL]) == int(cap is not None and r.ncon > cap), what
  return worst(errs), float(skip.mean())


# ---- tolerances -------------------------------------------------------------------------------------------------------------------
# fp64: the project's 1e-9; the ellipsoid pairs' pos and frame get the 1e-8 of tests/test_ellipsoid_collision.py (their
# iteration stops at ccd_tol, the last digits of the witness points depend on the summation order)
F64_TOL = {'analytic': dict.fromkeys(QUANTITIES, TOL_F64),
           'ellipsoid': dict(dist=TOL_F64, pos=1e-8, normal=1e-8, frame=1e-8)}
# fp32: the worst error per quantity and pair class measured on an MI355X against the oracle over the single-pair scenes
# (generic kernel, 64 and 16 lanes, sampled + directed poses; tests/test_gpu_contacts.py prints every figure); the bound
# is 4 x that, the rule of the ray and camera tests: the margin leaves room for the other scenes -- the heap, the suite
# models, the per-environment geoms -- whose worst figures are noted behind.  (None = not measured: the bound is then the
# ceiling.)  Ceilings: TOL_F32_ONE_STEP for the analytic pairs, the 2e-4 on dist / 2e-3 on pos and frame of
# tests/test_ellipsoid_collision.py for the ellipsoid pairs.
F32_MEASURED = {
    # capsule-box / capsule-cylinder / capsule-cylinder / capsule-cylinder  (other scenes: cheetah dist 2.106e-7, heap pos
    # 3.931e-7, stacker normal and frame 1.587e-5; host build: 1.24e-7 / 2.49e-7 / 4.69e-6 / 4.78e-6)
    'analytic': dict(dist=6.529e-8, pos=3.089e-7, normal=4.689e-6, frame=4.811e-6),
    # ellipsoid-ellipsoid / capsule-ellipsoid / capsule-ellipsoid / sphere-ellipsoid: the iteration stops at ccd_tol = 1e-4
    # (host build: 5.05e-8 / 9.50e-6 / 9.08e-5 / 9.78e-5)
    'ellipsoid': dict(dist=4.842e-8, pos=9.496e-6, normal=8.345e-5, frame=9.572e-5)}
F32_CEILING = {'analytic': dict.fromkeys(QUANTITIES, TOL_F32_ONE_STEP),
               'ellipsoid': dict(dist=2e-4, pos=2e-3, normal=2e-3, frame=2e-3)}
F32_TOL = {c: {k: F32_CEILING[c][k] if v is None else 4*v for k, v in F32_MEASURED[c].items()} for c in F32_MEASURED}
for _c in F32_TOL:
  for _k in QUANTITIES:
    assert F32_TOL[_c][_k] <= F32_CEILING[_c][_k], (_c, _k)


def tolerance(cls, prec):
  return (F64_TOL if prec == 64 else F32_TOL)[cls]


def assert_within(errs, cls, prec, what=''):
  tol = tolerance(cls, prec)
  for k in QUANTITIES:
    assert errs[k] <= tol[k], '%s fp%d: %s error %.3e exceeds %.1e' % (what, prec, k, errs[k], tol[k])

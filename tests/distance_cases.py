"""TEST INFRASTRUCTURE: the scene, states, pairs and bounds of the distance tests (CPU and GPU tiers).

Scene: a plane and ten free bodies, two of each convex primitive, one geom each at the body's origin (a geom's pose is its
body's).  Half-sizes, aspect ratios between 1.2 and 2.3:

  sphere     0.12 | 0.08                      capsule   r 0.08 h 0.14 | r 0.10 h 0.10
  ellipsoid  0.16 0.10 0.07 | 0.09 0.12 0.15  cylinder  r 0.09 h 0.12 | r 0.12 h 0.06
  box        0.12 0.08 0.06 | 0.07 0.10 0.13

Pairs: all 55 pairs of the 11 geoms in (i < j) order: 45 convex pairs (15 type pairs: one pair where the types are equal,
four where they differ) and 10 plane pairs (5 type pairs, two each).

States: 32 seeded states; state k draws every body's position uniformly in a cube of half-width SPREAD[k % 5] about
(0, 0, CENTRE_Z) and its orientation uniformly.  The tight cubes make cores overlap, the wide one separates.
Convergence at the default options (tolerance 1e-6, 50 iterations) is a condition on these inputs: about 0.2 % of such
random cases, all of them deep overlaps with an ellipsoid, need more than 50 EPA iterations (status 1).  State k
therefore uses SEEDS[k]: the first of 1000 + k + 100 j whose 55 pairs reach status 0 in the fp64 and the fp32 host build
(j = 0 for 27 of the 32 states; chosen by scripts/make_distance_golden.py --seeds).  Nothing is excluded at run time.

Classes of a case, from the twin's distance d and the rounding radii r1 + r2 of the pair (sphere, capsule: size[0]):
  apart    d > 0
  shallow  -(r1 + r2) < d <= 0      only where r1 + r2 > 0: the pair has a sphere or a capsule
  deep     d <= -(r1 + r2)          cores overlap (EPA); impossible for sphere-sphere, sphere-capsule, capsule-capsule
                                    (two points / segments meet with probability zero) and undefined against a plane
MIX_MIN of the cases of every type pair fall in each class the table below allows.
"""
import itertools
import os

import numpy as np

import dist_twin as tw

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'distance_cases.npz')
NSTATE = 32
SPREAD = (0.05, 0.10, 0.17, 0.26, 0.45)
CENTRE_Z = 0.12
MIX_MIN = 0.20
DISTMAX = 10.0
TOLERANCE, ITERATIONS = 1e-6, 50
TOL_F64 = 1e-9                 # the project's fp64 bound, x max(1, |d|): pairs whose cores are points, segments or boxes
TOL_F32_ONE_STEP = 5e-5        # the project's fp32 one-step tolerance
UNIQUE_REL = 1e-3              # a second local optimum within this (relative) of the best: the witness is not unique
UNIQUE_CAP = 0.05              # at most this share of a type pair's random cases may be left out of the point comparison

GEOMS = [      # (name, type, size)
    ('floor', tw.PLANE, (0, 0, 0.1)),
    ('sph0', tw.SPHERE, (0.12, 0, 0)), ('sph1', tw.SPHERE, (0.08, 0, 0)),
    ('cap0', tw.CAPSULE, (0.08, 0.14, 0)), ('cap1', tw.CAPSULE, (0.10, 0.10, 0)),
    ('ell0', tw.ELLIPSOID, (0.16, 0.10, 0.07)), ('ell1', tw.ELLIPSOID, (0.09, 0.12, 0.15)),
    ('cyl0', tw.CYLINDER, (0.09, 0.12, 0)), ('cyl1', tw.CYLINDER, (0.12, 0.06, 0)),
    ('box0', tw.BOX, (0.12, 0.08, 0.06)), ('box1', tw.BOX, (0.07, 0.10, 0.13)),
]
_TYPE_NAME = {tw.PLANE: 'plane', tw.SPHERE: 'sphere', tw.CAPSULE: 'capsule', tw.ELLIPSOID: 'ellipsoid', tw.CYLINDER: 'cylinder', tw.BOX: 'box'}
PAIRS = list(itertools.combinations(range(len(GEOMS)), 2))      # 55
NBODY = len(GEOMS) - 1
ROUND = (tw.SPHERE, tw.CAPSULE)
EXACT_TYPES = (tw.PLANE, tw.SPHERE, tw.CAPSULE, tw.BOX)      # cores that are points, segments or boxes (a plane: closed form)


def type_pair(p):
  return tuple(sorted((GEOMS[p[0]][1], GEOMS[p[1]][1])))


TYPE_PAIRS = sorted({type_pair(p) for p in PAIRS})      # 20


def classes_allowed(tp):
  if tw.PLANE in tp:
    return ('apart', 'overlap')
  if tp[0] in ROUND and tp[1] in ROUND:
    return ('apart', 'shallow')
  if tp[0] in ROUND or tp[1] in ROUND:
    return ('apart', 'shallow', 'deep')
  return ('apart', 'deep')


def radii(p):
  return sum(GEOMS[g][2][0] for g in p if GEOMS[g][1] in ROUND)


def classify(p, d):
  if tw.PLANE in type_pair(p):
    return 'apart' if d > 0 else 'overlap'
  r = radii(p)
  return 'apart' if d > 0 else 'shallow' if d > -r else 'deep'


def exact_pair(p):
  return all(GEOMS[g][1] in EXACT_TYPES for g in p)


def xml(margin=None, extra='', collide=True):
  """The scene; collide=False switches every geom's contacts off (contype = conaffinity = 0): the device's step kernel
  refuses a model whose pair list holds ellipsoid-box, box / ellipsoid against a cylinder or cylinder-cylinder."""
  def geom(name, t, s):
    size = {tw.PLANE: '2 2 0.1', tw.SPHERE: '%g' % s[0], tw.CAPSULE: '%g %g' % s[:2], tw.CYLINDER: '%g %g' % s[:2]}.get(t, '%g %g %g' % tuple(s))
    return '<geom name="%s" type="%s" size="%s"%s%s/>' % (name, _TYPE_NAME[t], size, '' if margin is None else ' margin="%g"' % margin,
                                                          '' if collide else ' contype="0" conaffinity="0"')
  bodies = ''.join('<body name="b_%s" pos="%g 0 0.5"><freejoint/>%s</body>' % (n, 0.5*i, geom(n, t, s))
                   for i, (n, t, s) in enumerate(GEOMS[1:]))
  return '<mujoco><option gravity="0 0 0"/><worldbody>%s%s%s</worldbody></mujoco>' % (geom(*GEOMS[0]), bodies, extra)


SEEDS = (1000, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1008, 1009, 1210, 1011, 1112, 1013, 1014, 1215, 1016, 1017, 1018, 1019, 1120,
         1021, 1022, 1023, 1024, 1025, 1026, 1027, 1028, 1029, 1230, 1031)

# Cases of the seeds that were passed over: (state k, seed, pair) that end at status 1 under the default options in the fp64
# host build -- deep overlaps with an ellipsoid whose depth is nearly flat over the directions.  They are checked as what
# they are: status nonzero, dist an attained value (never above the truth by more than the twin's error) and within the
# gap the solver itself certified (DistResult.gap; measured errors 3.5e-6 .. 5.0e-5, gaps 4.2e-5 .. 1.0e-3).
STATUS1_CASES = ((10, 1010, (5, 6)), (10, 1010, (5, 8)), (12, 1012, (3, 6)), (20, 1020, (5, 6)), (30, 1130, (5, 6)))


def random_state(k, seed=None):
  """(pos (10, 3), quat (10, 4)) of state k."""
  rs = np.random.RandomState(SEEDS[k] if seed is None else seed)
  L = SPREAD[k % len(SPREAD)]
  pos = rs.uniform(-L, L, (NBODY, 3)) + [0, 0, CENTRE_Z]
  q = rs.normal(size=(NBODY, 4))
  return pos, q / np.linalg.norm(q, axis=1, keepdims=True)


def aligned_states():
  """A handful of exactly axis-aligned states: the non-unique-witness cases.  Every body far apart on a grid except the
  ones each state poses: box faces parallel (apart, overlapping), a cylinder cap on a box face, a capsule lying along a box
  face, a box flat on the plane."""
  out = []
  idx = {n: i - 1 for i, (n, _, _) in enumerate(GEOMS) if i}
  for k in range(5):
    pos = np.array([[3.0*(i + 1), 0, 2.0] for i in range(NBODY)])
    q = np.tile([1.0, 0, 0, 0], (NBODY, 1))
    if k == 0:      # box faces parallel, apart along x, offset in y
      pos[idx['box0']] = [0, 0, 1]; pos[idx['box1']] = [0.3, 0.05, 1]
    elif k == 1:    # boxes overlapping, axes parallel
      pos[idx['box0']] = [0, 0, 1]; pos[idx['box1']] = [0.15, 0.02, 1.01]
    elif k == 2:    # a cylinder's cap above a box face, apart; then the other cylinder sunk into the other box
      pos[idx['box0']] = [0, 0, 1]; pos[idx['cyl0']] = [0.02, 0.01, 1.25]
      pos[idx['box1']] = [0, 2, 1]; pos[idx['cyl1']] = [0.01, 2, 1.15]
    elif k == 3:    # a capsule lying along a box face (axis parallel to it)
      pos[idx['box0']] = [0, 0, 1]; pos[idx['cap0']] = [0.25, 0, 1]
    else:           # a box flat on the plane, a cylinder standing on it
      pos[idx['box0']] = [0, 0, 0.05]; pos[idx['cyl0']] = [1, 0, 0.2]
    out.append((pos, q))
  return out


def states():
  """Every state: the 32 random ones, then the aligned ones.  (pos (S, 10, 3), quat (S, 10, 4), aligned (S,) bool)."""
  st = [random_state(k) for k in range(NSTATE)] + aligned_states()
  return (np.array([s[0] for s in st]), np.array([s[1] for s in st]), np.arange(len(st)) >= NSTATE)


def geoms_of(pos, quat):
  """The 11 twin geoms of one state."""
  g = [tw.Geom(GEOMS[0][1], GEOMS[0][2], (0, 0, 0), np.eye(3))]
  return g + [tw.Geom(t, s, pos[i], tw.quat_to_mat(quat[i])) for i, (_, t, s) in enumerate(GEOMS[1:])]


def qpos_of(pos, quat):
  return np.concatenate([pos, quat], axis=-1).reshape(pos.shape[:-2] + (-1,))


def twin_case(geoms, p):
  """(dist, fromto (6,), unique, gap) of pair p from the twin."""
  r = tw.distance(geoms[p[0]], geoms[p[1]])
  unique = not (r['second'] >= r['dist'] - UNIQUE_REL*abs(r['dist']))
  return r['dist'], r['fromto'], unique, r['gap']


def load_golden():
  z = np.load(GOLDEN)
  return {k: z[k] for k in z.files}


# fp32 against the twin: the worst |d - d_twin| / max(1, |d_twin|) of the fp32 HOST build over the fixture, measured by
# scripts/make_distance_golden.py (profiles/distance_accuracy.json); the test's bound is 4 x that.  E_TWIN: the twin's own
# worst error against the closed forms, same file.
F32_MEASURED = 3.748e-6      # a deep capsule-ellipsoid overlap; pairs of points, segments and boxes: 1.4e-7
E_TWIN = 1.87e-14
F32_TOL = 4*F32_MEASURED
assert F32_TOL <= TOL_F32_ONE_STEP
# Witness points against the twin, where it marks them unique.  A witness is less certain than the distance: on a surface
# of curvature radius R an error e of the distance moves the closest point sideways by up to sqrt(2 R e).  With R <= 1 (the
# scene is smaller) and e the solver's gap, tolerance max(1, |d|) = 1e-6 in fp64 and its floor of 32 machine epsilons in
# fp32 plus the measured fp32 error, that is sqrt(2e-6) and sqrt(2 (3.8e-6 + F32_TOL)).
WITNESS_TOL = {64: (2*1e-6)**0.5, 32: (2*(3.82e-6 + F32_TOL))**0.5}
# The oracle's narrow phase returns the geometric distance (its contact `dist`, inside a large margin) for these type
# pairs: every collider with a plane, and the closed-form or exact colliders among spheres, capsules, ellipsoids and
# cylinders.  Left out: box-box (SAT: not the Euclidean distance while apart), capsule-box (the oracle's collider picks
# the nearest box feature approximately) and the pairs the oracle refuses (ellipsoid-box, box / ellipsoid against a
# cylinder, cylinder-cylinder).
ORACLE_PIN_TYPES = ((0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (2, 2), (2, 3), (2, 4), (2, 5), (2, 6), (3, 3), (3, 4), (3, 5), (4, 4))

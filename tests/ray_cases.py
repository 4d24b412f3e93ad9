"""TEST INFRASTRUCTURE: the scene, states and ray sets of the ray tests (CPU and GPU tiers)."""
import numpy as np

import camera_scenes as cs
from dm_control_amd import mjcf_compiler as mc

EDGE_CAP = 0.03      # the project's cap on the share of rays the edge rule may exclude
TOL_F64 = 1e-9
TOL_F32_ONE_STEP = 5e-5      # the project's fp32 one-step tolerance: the fp32 ray bound must stay below it
RING_ELEVATIONS = (-0.6, -0.25, 0.0)
RING_AZIMUTHS = 32
NSTATE = 3


def model(sites=''):
  return mc.compile_xml(cs.six_primitive_xml(sites))


def state_qpos(m, k):
  """State k of the six-primitive scene: the ball displaced, the arm swung."""
  q = np.array(m.qpos0, dtype=np.float64)
  q[:3] += [0.1*k, -0.15*k, 0.2*k]
  q[7] = 0.6*k
  return q


def seeded_rays(k, n=256):
  """Set (a): n seeded rays of state k with non-unit directions."""
  rs = np.random.RandomState(7 + k)
  origin = rs.uniform([-1.2, -1.1, 0.05], [1.2, 1.1, 1.4], (n, 3))
  target = rs.uniform([-0.9, -0.8, 0.0], [0.9, 0.8, 0.7], (n, 3))
  return origin, (target - origin) * rs.uniform(0.3, 2.0, (n, 1))


def ring_dirs():
  """Set (b): 3 elevations x 32 azimuths at 2 pi (i + 0.5) / 32, unit vectors, elevation-major."""
  az = 2*np.pi*(np.arange(RING_AZIMUTHS) + 0.5)/RING_AZIMUTHS
  return np.concatenate([np.stack([np.cos(e)*np.cos(az), np.cos(e)*np.sin(az), np.full(az.shape, np.sin(e))], 1)
                         for e in RING_ELEVATIONS], 0)


def ring_rays(m, xpos, xmat):
  """Set (b) in the world frame for one environment: from body `ball`, in its frame."""
  b = m.name2id('ball', 'body')
  R = np.asarray(xmat, dtype=np.float64).reshape(-1, 3, 3)[b]
  d = ring_dirs() @ R.T
  return np.tile(np.asarray(xpos, dtype=np.float64).reshape(-1, 3)[b], (len(d), 1)), d


def rel_error(x, ref, vec):
  """|dx| |vec| / max(1, x |vec|), the bound form of the ray tests."""
  n = np.linalg.norm(vec, axis=1)
  return np.abs(x - ref)*n / np.maximum(1.0, ref*n)


def rig_sites(m0, pnt, vec):
  """(sites, sensors) XML: one site + rangefinder per world ray on the geom-less static body `rig`."""
  rig = m0.name2id('rig', 'body')
  import camera_twin as twin
  Rr = twin.quat_to_mat(m0.body_quat[rig])
  lp = (np.asarray(pnt) - m0.body_pos[rig]) @ Rr
  lz = (np.asarray(vec) / np.linalg.norm(vec, axis=1, keepdims=True)) @ Rr
  sites = ''.join('<site name="ray%d" pos="%s" zaxis="%s"/>' % (i, ' '.join(repr(float(v)) for v in lp[i]), ' '.join(repr(float(v)) for v in lz[i]))
                  for i in range(len(lp)))
  sensors = '<sensor>%s</sensor>' % ''.join('<rangefinder site="ray%d"/>' % i for i in range(len(lp)))
  return sites, sensors


def rangefinder_rays(m0):
  """The 48-ray subset the rangefinder comparisons use: the first 32 rays of set (a), state 0, and every sixth ray of
  set (b) from the ball's position at qpos0 -- world rays, the same in every state."""
  o, v = seeded_rays(0)
  ball = m0.name2id('ball', 'body')
  ro = np.tile(np.asarray(m0.body_pos[ball], dtype=np.float64), (16, 1))
  return np.concatenate([o[:32], ro], 0), np.concatenate([v[:32], ring_dirs()[::6]], 0)


# fp32: the maximum of |dx| |vec| / max(1, x |vec|) measured on an MI355X against the twin over sets (a) and (b), states
# 0..2, cast and scan kernels (tests/test_gpu_rays.py prints it); the bound is 4 x that, the camera test's rule: the margin
# leaves room for other states.  (None = not measured: the bound is then TOL_F32_ONE_STEP alone.)
F32_MEASURED = 2.605e-7      # set (a), state 0, cast kernel; the scan kernel on set (b): 2.4e-7 (host build: 3.4e-7 / 2.4e-7)
F32_TOL = TOL_F32_ONE_STEP if F32_MEASURED is None else 4*F32_MEASURED
assert F32_TOL <= TOL_F32_ONE_STEP

"""The two ray codes against each other on the host (tests/emu/geom_emu.cpp: only step_geom.h and camera_core.h).

The step kernel's rangefinder rays (step_geom.h ray_geom_any: textbook discriminant on a world-frame pose) and the
camera's (camera_core.h cam_ray_local: roots through the point of closest approach, behind the camera's own
pre-transform) are two texts of the same closed forms, kept apart for the numerical reason DESIGN.md gives ("Ray code").
This pins them together in fp64: every primitive type, 200 seeded rays each, origins outside at 3 .. 10 bounding radii
from the geom; half the rays aim at a point inside the primitive at no more than 0.8 of its half-sizes (certain hits), half
point directly away from such a point (certain misses); none grazes, so none is excluded.  Hit / miss must agree on all of
them and the distances within 1e-9 max(1, t), the bound DESIGN.md records for the camera twin against the oracle's rays.
"""
import ctypes
import os

import numpy as np
import pytest

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = 0, 2, 3, 4, 5, 6      # include/dmc_model_layout.h DMC_GEOM_*
TYPES = {'plane': PLANE, 'sphere': SPHERE, 'capsule': CAPSULE, 'ellipsoid': ELLIPSOID, 'cylinder': CYLINDER, 'box': BOX}
NRAYS = 200


@pytest.fixture(scope='module')
def rays(tmp_path_factory):
  lib = host_build.load(os.path.join(ROOT, 'tests', 'emu', 'geom_emu.cpp'), 'geom_emu', out_dir=str(tmp_path_factory.mktemp('geom_emu')))
  lib.geom_emu_rays.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 8
  lib.geom_emu_rays.restype = None

  def run(typ, size, gpos, gmat, pnt, vec):
    n = len(typ)
    a = [np.ascontiguousarray(typ, dtype=np.int32)] + [np.ascontiguousarray(x, dtype=np.float64) for x in (size, gpos, gmat, pnt, vec)]
    t_step, t_cam = np.zeros(n), np.zeros(n)
    lib.geom_emu_rays(n, *[x.ctypes.data for x in a], t_step.ctypes.data, t_cam.ctypes.data)
    return t_step, t_cam
  return run


def _unit(rs, n):
  v = rs.normal(size=(n, 3))
  return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rotations(rs, n):
  q = rs.normal(size=(n, 4))
  w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
  return np.stack([1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y),
                   2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x),
                   2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)], 1).reshape(n, 3, 3)


def _case(name, seed):
  """(type, size, gpos, gmat, pnt, vec, expect_hit): the first half of the rays are the certain hits."""
  typ, n = TYPES[name], NRAYS
  rs = np.random.RandomState(seed)
  size = rs.uniform(0.2, 1.0, (n, 3))
  gpos = rs.uniform(-2, 2, (n, 3))
  R = _rotations(rs, n)
  # a point inside the primitive, in its frame, at no more than 0.8 of its half-sizes; the bounding radius
  ball = _unit(rs, n) * rs.uniform(0, 1, (n, 1)) ** (1 / 3)
  disc = ball[:, :2] / np.maximum(1e-12, np.linalg.norm(ball[:, :2], axis=1, keepdims=True)) * np.sqrt(rs.uniform(0, 1, (n, 1)))
  cube = rs.uniform(-1, 1, (n, 3))
  if typ == SPHERE:
    inside, rb = 0.8 * size[:, :1] * ball, size[:, 0]
  elif typ == ELLIPSOID:
    inside, rb = 0.8 * size * ball, size.max(1)
  elif typ == CAPSULE:
    inside, rb = 0.8 * np.concatenate([size[:, :1] * disc, size[:, 1:2] * cube[:, 2:]], 1), size[:, 0] + size[:, 1]
  elif typ == CYLINDER:
    inside, rb = 0.8 * np.concatenate([size[:, :1] * disc, size[:, 1:2] * cube[:, 2:]], 1), np.hypot(size[:, 0], size[:, 1])
  elif typ == BOX:
    inside, rb = 0.8 * size * cube, np.linalg.norm(size, axis=1)
  else:      # a finite plane: hit from its front side only
    inside, rb = 0.8 * np.concatenate([size[:, :2] * cube[:, :2], np.zeros((n, 1))], 1), np.hypot(size[:, 0], size[:, 1])
  out = _unit(rs, n)
  if typ == PLANE:
    out[:, 2] = np.abs(out[:, 2]) + 0.5      # well above the plane: no grazing incidence
    out /= np.linalg.norm(out, axis=1, keepdims=True)
  origin = out * (rs.uniform(3, 10, n) * rb)[:, None]
  aim = inside - origin
  aim /= np.linalg.norm(aim, axis=1, keepdims=True)
  hit = np.arange(n) < n // 2
  aim[~hit] *= -1
  world = lambda v: np.einsum('nij,nj->ni', R, v)
  return np.full(n, typ), size, gpos, R.reshape(n, 9), gpos + world(origin), world(aim), hit


@pytest.mark.parametrize('name', sorted(TYPES))
def test_step_rays_match_camera_rays(rays, name):
  typ, size, gpos, gmat, pnt, vec, hit = _case(name, 1234 + TYPES[name])
  t_step, t_cam = rays(typ, size, gpos, gmat, pnt, vec)
  assert np.array_equal(t_step >= 0, hit), 'ray_geom_any: hit / miss'
  assert np.array_equal(t_cam >= 0, hit), 'cam_ray_local: hit / miss'
  d = np.abs(t_step - t_cam)[hit]
  print('%s: max |t_step - t_cam| = %.3e over %d hits (t up to %.2f)' % (name, d.max(), hit.sum(), t_step[hit].max()))
  assert np.all(d <= 1e-9 * np.maximum(1, t_step[hit]))
  assert np.all(t_step[~hit] == -1) and np.all(t_cam[~hit] == -1)

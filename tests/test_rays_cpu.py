"""Batched ray casts, CPU tier: the numpy twin (tests/ray_twin.py) against the unchanged fp64 oracle's rangefinder rays,
the host build of the kernels' per-ray functions (tests/emu/ray_emu.cpp: csrc/ray_core.h in fp32 and fp64) against the
twin and against the step kernel's ray_geom_any, the filter rules, mujoco_api.mj_ray on the oracle stand-in, and what
BatchRays / lidar.wrap check before they touch a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import camera_twin
import ray_cases as rc
import ray_emu_lib as emu
import ray_twin as rt
from dm_control_amd import host_data
from dm_control_amd import rays
from oracle.oracle import OraclePhysics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_state(m, k):
  p = OraclePhysics(m)
  p.qpos[:] = rc.state_qpos(m, k)
  p.forward()
  return p


@pytest.fixture(scope='module')
def scene():
  """The model, and per state the oracle's poses with the twin's answers for sets (a) and (b): computed once, shared."""
  m = rc.model()
  ball = m.name2id('ball', 'body')
  states = []
  for k in range(rc.NSTATE):
    p = oracle_state(m, k)
    st = dict(gpos=np.array(p.geom_xpos, dtype=np.float64), gmat=np.array(p.geom_xmat, dtype=np.float64),
              xpos=np.array(p.xpos, dtype=np.float64).reshape(-1, 3), xmat=np.array(p.xmat, dtype=np.float64).reshape(-1, 3, 3))
    st['sets'] = {}
    for name, (o, v), bex in (('a', rc.seeded_rays(k), -1), ('b', rc.ring_rays(m, st['xpos'], st['xmat']), ball)):
      st['sets'][name] = dict(pnt=o, vec=v, bex=bex, twin=rt.cast(m, st['gpos'], st['gmat'], o, v, bodyexclude=bex))
    states.append(st)
  return m, states


def test_twin_equals_the_oracles_rangefinder_rays():
  m0 = rc.model()
  pnt, vec = rc.rangefinder_rays(m0)
  assert len(pnt) == 48
  m = rc.model(rc.rig_sites(m0, pnt, vec))
  rig = m.name2id('rig', 'body')
  assert m.body_geomnum[rig] == 0      # (a rangefinder skips its own body's geoms: none here)
  seen = set()
  for k in range(rc.NSTATE):
    p = oracle_state(m, k)
    tw = rt.cast(m, p.geom_xpos, p.geom_xmat, pnt, vec, bodyexclude=rig, geomgroup=None, flg_static=1, edge=False)
    sd = np.array(p.sensordata, dtype=np.float64)
    metres = np.where(tw['gid'] >= 0, tw['dist']*np.linalg.norm(vec, axis=1), -1.0)      # x is in units of |vec|
    assert np.array_equal(sd < 0, tw['gid'] < 0)
    assert np.all(sd[tw['gid'] < 0] == -1) and np.all(tw['dist'][tw['gid'] < 0] == -1)      # misses are -1 in both
    np.testing.assert_allclose(metres, sd, rtol=0, atol=1e-9)
    seen |= set(int(m.geom_type[g]) for g in tw['gid'][tw['gid'] >= 0])
    assert m.name2id('ghost', 'geom') not in tw['gid']
  assert seen == set(camera_twin.DRAWN), seen      # every primitive type was hit somewhere


@pytest.mark.parametrize('name', ['a', 'b'])
def test_edge_rule_stays_under_the_cap(scene, name):
  m, states = scene
  for k, st in enumerate(states):
    share = st['sets'][name]['twin']['excluded'].mean()
    print('set (%s) state %d: excluded %.4f' % (name, k, share))
    assert share <= rc.EDGE_CAP, (name, k, share)


@pytest.mark.parametrize('prec,tol', [(64, rc.TOL_F64), (32, rc.F32_TOL)])
def test_host_build_of_ray_core_equals_the_twin(scene, prec, tol):
  m, states = scene
  ok = rt.hittable(m)
  worst = 0.0
  for k, st in enumerate(states):
    for name, s in st['sets'].items():
      tw, keep = s['twin'], ~s['twin']['excluded']
      d, g, n = emu.cast(prec, m, ok, st['gpos'], st['gmat'], s['pnt'], s['vec'], s['bex'])
      assert np.array_equal(g[keep], tw['gid'][keep]), (prec, k, name)
      assert np.all(d[keep & (tw['gid'] < 0)] == -1)
      hit = keep & (tw['gid'] >= 0)
      assert hit.sum() > 15
      err = rc.rel_error(d[hit], tw['dist'][hit], s['vec'][hit])
      worst = max(worst, err.max())
      assert np.abs(n[hit] - tw['normal'][hit]).max() < (1e-9 if prec == 64 else 1e-3), (prec, k, name)
      np.testing.assert_allclose(np.linalg.norm(n[hit], axis=1), 1.0, atol=1e-6)
      if name == 'b':      # the scan kernel's arithmetic: frame pose, ray-ready geoms, directions in the ball's frame
        b = s['bex']
        ds, gs = emu.scan(prec, m, ok, st['gpos'], st['gmat'], rays.FRAME_BODY, st['xpos'][b], st['xmat'][b], (0, 0, 0), rc.ring_dirs(), b)
        assert np.array_equal(gs[keep], tw['gid'][keep]), (prec, k)
        worst = max(worst, rc.rel_error(ds[hit], tw['dist'][hit], s['vec'][hit]).max())
  print('fp%d host build: max |dx| |vec| / max(1, x |vec|) = %.4g' % (prec, worst))
  assert worst <= tol, worst


def test_host_build_of_ray_core_equals_ray_geom_any(scene):
  m, states = scene
  ok = rt.hittable(m)
  worst = 0.0
  for st in states:
    for s in st['sets'].values():
      keep = ~s['twin']['excluded']
      d, g, _ = emu.cast(64, m, ok, st['gpos'], st['gmat'], s['pnt'], s['vec'], s['bex'])
      ds, gs, _ = emu.cast(64, m, ok, st['gpos'], st['gmat'], s['pnt'], s['vec'], s['bex'], step=True)
      assert np.array_equal(g[keep], gs[keep])
      assert np.all(ds[keep & (g < 0)] == -1)
      hit = keep & (g >= 0)
      worst = max(worst, rc.rel_error(d[hit], ds[hit], s['vec'][hit]).max())
  print('ray_core.h against ray_geom_any: %.4g' % worst)
  assert worst <= 1e-12


def _all(m, st, pnt, vec, **kw):
  """One question asked of the twin, the host build (fp64) and host_data.ray_cast: they must agree; returns the twin's."""
  pnt, vec = np.atleast_2d(np.asarray(pnt, dtype=np.float64)), np.atleast_2d(np.asarray(vec, dtype=np.float64))
  tw = rt.cast(m, st['gpos'], st['gmat'], pnt, vec, edge=False, **kw)
  bex = np.broadcast_to(np.asarray(kw.get('bodyexclude', -1)), (len(vec),))
  d, g, _ = emu.cast(64, m, rt.hittable(m, kw.get('geomgroup'), kw.get('flg_static', 1)), st['gpos'], st['gmat'], pnt, vec, bex,
                     cutoff=kw.get('cutoff'))
  assert np.array_equal(g, tw['gid']) and np.allclose(d, tw['dist'], rtol=0, atol=1e-9)
  if kw.get('cutoff') is None:
    for i in range(len(vec)):
      x, gi = host_data.ray_cast(m, st['gpos'], st['gmat'], m.geom_size, pnt[i], vec[i], kw.get('geomgroup'), kw.get('flg_static', 1), int(bex[i]))
      assert gi == tw['gid'][i] and abs(x - tw['dist'][i]) <= 1e-9
  return tw['dist'], tw['gid']


def test_filters(scene):
  m, states = scene
  st = states[0]
  gid = lambda n: m.name2id(n, 'geom')
  down = [0, 0, -1.0]
  # `hidden` (group 3) sits on the floor at the origin: hit with every group, passed through with groups 0..2 only
  d, g = _all(m, st, [0, 0, 1.0], down, geomgroup=None)
  assert g[0] == gid('hidden') and abs(d[0] - 0.76) < 1e-12
  d, g = _all(m, st, [0, 0, 1.0], down, geomgroup=(1, 1, 1, 0, 0, 0))
  assert g[0] == gid('floor') and abs(d[0] - 1.0) < 1e-12
  assert np.array_equal(rt.hittable(m, (1, 1, 1, 0, 0, 0)), host_data.ray_filter(m, (1, 1, 1, 0, 0, 0), 1))
  # `ghost` (alpha 0) is never hit: a ray through its centre reaches the floor
  d, g = _all(m, st, [-0.9, -0.9, 1.5], down)
  assert g[0] == gid('floor') and abs(d[0] - 1.5) < 1e-12
  # flg_static = 0: only the geoms of moving bodies
  o, v = rc.seeded_rays(0)
  d, g = _all(m, st, o, v, flg_static=0)
  assert set(g) <= {-1, gid('ballg'), gid('armg')} and gid('ballg') in g and gid('armg') in g
  assert np.array_equal(rt.hittable(m, None, 0), host_data.ray_filter(m, None, 0))
  # bodyexclude per ray: the same ray down through the ball, once excluding it
  top = st['xpos'][m.name2id('ball', 'body')] + [0, 0, 0.5]
  d, g = _all(m, st, [top, top], [down, down], bodyexclude=np.array([-1, m.name2id('ball', 'body')]))
  assert g[0] == gid('ballg') and abs(d[0] - 0.4) < 1e-12 and g[1] != gid('ballg') and d[1] > d[0]
  # cutoff, in metres whatever |vec|: 0.4 m to the ball
  for scale in (1.0, 0.25, 3.0):
    v = np.array(down)*scale
    d, g = _all(m, st, top, v, cutoff=0.41)
    assert g[0] == gid('ballg') and abs(d[0]*scale - 0.4) < 1e-12      # x is in units of |vec|
    d, g = _all(m, st, top, v, cutoff=0.39, bodyexclude=-1)
    assert g[0] == -1 and d[0] == -1
  # a ray started inside `box` leaves through a face: along the box's own +x from its centre, 0.15 m
  b = gid('box')
  d, g = _all(m, st, st['gpos'].reshape(-1, 3)[b], st['gmat'].reshape(-1, 3, 3)[b][:, 0])
  assert g[0] == b and abs(d[0] - 0.15) < 1e-12
  # the plane: missed from behind, and beyond its finite size (1.6 x 1.4)
  d, g = _all(m, st, [1.0, 1.0, -0.5], [0, 0, 1.0])
  assert g[0] != gid('floor')
  d, g = _all(m, st, [1.7, 0, 0.5], down)
  assert g[0] == -1 and d[0] == -1
  d, g = _all(m, st, [1.5, 0, 0.5], down)
  assert g[0] == gid('floor')


def test_mj_ray_on_the_oracle_stand_in(monkeypatch, scene):
  import oracle_backend as ob
  import camera_scenes as cs
  from dm_control_amd import mujoco_api as mj
  monkeypatch.setattr(mj, 'BatchedPhysics', ob.OracleBatch)      # (the facade on the CPU oracle)
  m, states = scene
  model = mj.MjModel.from_xml_string(cs.six_primitive_xml())
  data = mj.MjData(model)
  data.qpos[:] = rc.state_qpos(m, 1)
  mj.mj_forward(model, data)
  st = states[1]
  o, v = rc.seeded_rays(1, 24)
  tw = rt.cast(m, st['gpos'], st['gmat'], o, v, edge=False)
  assert (tw['gid'] >= 0).any() and (tw['gid'] < 0).any()
  for i in range(len(o)):
    geomid = np.full(1, -7, dtype=np.int32)
    x = mj.mj_ray(model, data, o[i], v[i], None, 1, -1, geomid)      # the maze's call pattern (random_goal_maze.py:179-187)
    assert isinstance(x, float) and geomid[0] == tw['gid'][i]
    assert abs(x - tw['dist'][i]) <= 1e-9*max(1.0, abs(tw['dist'][i]))
  # the other arguments reach the filter
  ball = m.name2id('ball', 'body')
  top = st['xpos'][ball] + [0, 0, 0.5]
  geomid = np.zeros(1, dtype=np.int32)
  assert abs(mj.mj_ray(model, data, top, [0, 0, -2.0], None, 1, -1, geomid) - 0.2) < 1e-9 and geomid[0] == m.name2id('ballg', 'geom')
  assert mj.mj_ray(model, data, top, [0, 0, -2.0], None, 1, ball, geomid) > 0.2 and geomid[0] != m.name2id('ballg', 'geom')
  assert mj.mj_ray(model, data, [0, 0, 1.0], [0, 0, -1.0], np.array([1, 1, 1, 0, 0, 0], dtype=np.uint8), 1, -1, geomid) == pytest.approx(1.0)
  assert geomid[0] == m.name2id('floor', 'geom')
  assert mj.mj_ray(model, data, [0, 0, 1.0], [0, 0, 1.0], None, 1, -1, geomid) == -1 and geomid[0] == -1
  assert mj.mj_ray(model, data, [0, 0, 1.0], [0, 0, -1.0], None, 0, -1, None) == -1      # geomid may be None


def test_ring_and_frames_and_broadcasting_need_no_device():
  import torch
  m = rc.model()
  # the full ring starts at azimuth -pi: set (b)'s table (which starts at 0), each elevation's row rolled by half a turn
  full = rays.ring(32, rc.RING_ELEVATIONS).reshape(3, 32, 3)
  np.testing.assert_allclose(np.roll(full, -16, axis=1), rc.ring_dirs().reshape(3, 32, 3), atol=1e-15)
  r = rays.ring(8, fov=math.pi)
  np.testing.assert_allclose(np.linalg.norm(r, axis=1), 1.0, atol=1e-15)
  assert r.shape == (8, 3) and np.all(r[:, 0] > 0) and np.all(r[:, 2] == 0)      # a half circle about +x
  for bad in (dict(n_azimuth=0), dict(n_azimuth=4, elevations=()), dict(n_azimuth=4, elevations=(2.0,)), dict(n_azimuth=4, fov=0.0)):
    with pytest.raises(ValueError):
      rays.ring(**bad)
  f = rays.resolve_frame(m, 'world')
  assert (f['type'], f['body']) == (rays.FRAME_WORLD, -1)
  f = rays.resolve_frame(m, dict(body='ball'))
  assert (f['type'], f['id'], f['body']) == (rays.FRAME_BODY, m.name2id('ball', 'body'), m.name2id('ball', 'body'))
  f = rays.resolve_frame(m, dict(geom='armg'))
  assert (f['type'], f['id'], f['body']) == (rays.FRAME_GEOM, m.name2id('armg', 'geom'), m.name2id('arm', 'body'))
  f = rays.resolve_frame(m, dict(camera='eye'))      # a fixed camera: its body's frame and a constant pose in it
  assert (f['type'], f['id']) == (rays.FRAME_BODY, m.name2id('rig', 'body'))
  np.testing.assert_allclose(f['pos'], (0.05, -0.02, 0.1))
  np.testing.assert_allclose(f['mat'], camera_twin.quat_to_mat((0.8804762, 0.4402381, -0.1320714, -0.1188643)), atol=1e-12)
  for bad in ('torso', dict(body='nobody'), dict(camera='track'), dict(body=99), dict(body=0, site=0), 3):
    with pytest.raises((ValueError, KeyError)):
      rays.resolve_frame(m, bad)
  assert rays.resolve_body(m, 'ball') == m.name2id('ball', 'body') and rays.resolve_body(m, -1) == -1
  with pytest.raises(ValueError):
    rays.resolve_body(m, m.nbody)
  # broadcasting: (3,), (R, 3) and (B, R, 3) in any mix
  p, v = rays.broadcast_rays(torch.zeros(3), torch.ones(5, 3), 4)
  assert tuple(p.shape) == tuple(v.shape) == (4, 5, 3) and p.is_contiguous() and v.is_contiguous()
  p, v = rays.broadcast_rays(np.zeros((4, 1, 3)), np.ones(3), 4, dtype=torch.float32)
  assert tuple(p.shape) == (4, 1, 3) and v.dtype == torch.float32
  p, v = rays.broadcast_rays(torch.arange(24.).reshape(4, 2, 3), torch.ones(2, 3), 4)
  assert tuple(v.shape) == (4, 2, 3) and torch.equal(p, torch.arange(24.).reshape(4, 2, 3))
  for bad in ((torch.zeros(2), torch.zeros(3)), (torch.zeros(5, 3), torch.zeros(4, 3)), (torch.zeros(3, 2, 3), torch.zeros(3)),
              (torch.zeros(1, 1, 1, 3), torch.zeros(3))):
    with pytest.raises(ValueError):
      rays.broadcast_rays(bad[0], bad[1], 4)


def test_argument_errors_need_no_device():
  from dm_control_amd.suite import lidar
  with pytest.raises(TypeError, match='BatchedPhysics'):
    rays.BatchRays(object())
  with pytest.raises(ValueError, match='scale'):
    lidar.wrap(object(), 'world', rays.ring(4), scale='log')
  with pytest.raises(ValueError, match='cutoff'):
    lidar.wrap(object(), 'world', rays.ring(4), scale='tanh')
  with pytest.raises(ValueError, match='directions'):
    lidar.wrap(object(), 'world', np.zeros((4, 2)))
  with pytest.raises(ValueError, match='zero length'):
    lidar.wrap(object(), 'world', np.zeros((4, 3)))
  with pytest.raises(TypeError, match='BatchedPhysics'):
    lidar.wrap(object(), 'world', rays.ring(4))


def test_ray_header_symbols_are_exported_and_fail_loudly_without_a_batch():
  from dm_control_amd import build
  build.build()
  from dm_control_amd import _native
  with open(os.path.join(ROOT, 'include', 'dmc_ray.h')) as f:
    declared = set(re.findall(r'\b(dmc_rays_[a-z0-9_]+)\s*\(', f.read()))
  assert declared == set(_native.RAY_EXPORTS)
  L = _native.lib()
  assert not [n for n in sorted(declared) if not hasattr(L, n)]
  out = ctypes.c_void_p()
  buf = (ctypes.c_double * 16)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  assert L.dmc_rays_create(None, p, ctypes.byref(out)) != 0 and b'null' in L.dmc_last_error() and not out.value
  assert L.dmc_rays_cast(None, 1, p, p, -1, None, 0, p, None, None, None) != 0 and b'null' in L.dmc_last_error()
  assert L.dmc_rays_scan(None, p, None, None, None) != 0 and b'null' in L.dmc_last_error()
  assert L.dmc_rays_add_scan(None, 0, 0, p, -1, 1, p) != 0 and b'null' in L.dmc_last_error()
  L.dmc_rays_destroy(None)
  # ray_kernels.hip is a unit of the one library with its own header list; the entry points' unit is stale against the
  # ray headers it includes
  units = {u[0]: u for u in build._UNITS}
  assert 'ray_core.h' in units['ray_kernels.hip'][2] and 'camera_core.h' in units['ray_kernels.hip'][2]
  assert not set(units['ray_kernels.hip'][2]) & set(build.STEP_SOURCES) - {'../../include/dmc_model_layout.h'}
  own = {os.path.basename(p) for p in build._own_includes(os.path.join(build.CSRC, 'dmc_api.hip'))}
  assert {'ray_core.h', 'dmc_ray.h', 'camera_core.h', 'dmc_batch.h'} <= own

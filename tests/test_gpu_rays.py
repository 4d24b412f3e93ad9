"""Batched ray casts on the GPU: the cast and scan kernels against the numpy twin (tests/ray_twin.py), which is always fed
the device's own poses read back with `batch.get` -- only the rays are under test -- and against the step kernel's own
rangefinder sensors.

Measured on an MI355X over sets (a) and (b), states 0..2 (max |dx| |vec| / max(1, x |vec|) on non-excluded rays, against
the twin):
  fp64 batch: 7.1e-15; bound: the project's fp64 tolerance, 1e-9
  fp32 batch: 2.605e-7 (ray_cases.F32_MEASURED); bound 4 x the maximum = 1.042e-6, below TOL_F32_ONE_STEP (5e-5)
The lidar tests run other scenes (a floor metres away, a 46 m pitch) at the environments' own precision; their bound is the
project's fp32 one-step tolerance, TOL_F32_ONE_STEP, not the figure measured on the six-primitive scene.
"""
import numpy as np
import pytest

import camera_scenes as cs
import ray_cases as rc
import ray_twin as rt
from dm_control_amd import mjcf_compiler as mc

pytestmark = pytest.mark.gpu

STATE = ('geom_xpos', 'geom_xmat', 'xpos', 'xmat', 'site_xpos', 'site_xmat')
B = 3


def make_batch(model, precision, batch_size=B, **kw):
  from dm_control_amd.batch import BatchedPhysics
  return BatchedPhysics(model, batch_size, precision=precision, **kw)


def six_batch(precision, batch_size=B, model=None):
  """Environment e holds state e % 3 of the CPU tier, set with set('qpos') + forward()."""
  m = rc.model() if model is None else model
  b = make_batch(m, precision, batch_size)
  b.set('qpos', np.stack([rc.state_qpos(m, e % rc.NSTATE) for e in range(batch_size)]))
  b.forward()
  b.sync()
  return b


def read_state(b):
  import torch
  torch.cuda.synchronize()
  return {k: b.get(k) for k in STATE}


def tensor(b, a):
  import torch
  return torch.as_tensor(np.asarray(a), dtype=torch.float64 if b.precision == 64 else torch.float32, device='cuda')


def against_twin(m, st, e, pnt, vec, dist, gid, label, normal=None, **kw):
  """Ids equal and the cap held on environment e; returns the worst distance error on the non-excluded rays."""
  tw = rt.cast(m, st['geom_xpos'][e], st['geom_xmat'][e], pnt, vec, **kw)
  share = tw['excluded'].mean()
  print('%s env %d: excluded %.4f' % (label, e, share))
  assert share <= rc.EDGE_CAP, (label, e, share)
  keep = ~tw['excluded']
  assert np.array_equal(gid[keep], tw['gid'][keep]), (label, e)
  assert np.all(dist[keep & (tw['gid'] < 0)] == -1), (label, e)
  hit = keep & (tw['gid'] >= 0)
  if normal is not None:
    assert np.abs(normal[hit] - tw['normal'][hit]).max() < 1e-3 and np.all(normal[tw['gid'] < 0][keep[tw['gid'] < 0]] == 0)
  return float(rc.rel_error(dist[hit], tw['dist'][hit], np.asarray(vec)[hit]).max()) if hit.any() else 0.0


def cast_and_scan_worst(precision):
  """Set (a) through the cast kernel and set (b) through the scan kernel, B = 3; the worst error of both."""
  from dm_control_amd import rays
  b = six_batch(precision)
  m = b.model
  br = rays.BatchRays(b)
  sets = [rc.seeded_rays(e) for e in range(B)]
  dist, gid, normal = br.cast(tensor(b, np.stack([s[0] for s in sets])), tensor(b, np.stack([s[1] for s in sets])), normals=True)
  assert dist.dtype == tensor(b, 0.0).dtype and gid.dtype.is_floating_point is False and tuple(normal.shape) == (B, 256, 3)
  ball = m.name2id('ball', 'body')
  assert br.add_scan(dict(body='ball'), rc.ring_dirs()) == 0 and br.scans[0]['bodyexclude'] == ball      # as a rangefinder
  sd, sg = br.scan()
  assert tuple(sd.shape) == (B, 1, 96)
  st = read_state(b)
  dist, gid, normal, sd, sg = (t.cpu().numpy() for t in (dist, gid, normal, sd, sg))
  worst = 0.0
  for e in range(B):
    worst = max(worst, against_twin(m, st, e, sets[e][0], sets[e][1], dist[e], gid[e], 'fp%d cast (a)' % precision, normal[e]))
    o, v = rc.ring_rays(m, st['xpos'][e], st['xmat'][e])
    worst = max(worst, against_twin(m, st, e, o, v, sd[e, 0], sg[e, 0], 'fp%d scan (b)' % precision, bodyexclude=ball))
  print('fp%d: max |dx| |vec| / max(1, x |vec|) over sets (a) and (b) = %.4g' % (precision, worst))
  return worst


def test_fp64_cast_and_scan_equal_the_twin():
  assert cast_and_scan_worst(64) <= rc.TOL_F64


def test_fp32_cast_and_scan_equal_the_twin():
  worst = cast_and_scan_worst(32)
  assert worst <= rc.F32_TOL, worst


def test_fp64_equals_the_step_kernels_rangefinders():
  """The scene compiled with 48 rangefinder sites on the geom-less body `rig`: the step kernel's own sensordata."""
  from dm_control_amd import rays
  m0 = rc.model()
  pnt, vec = rc.rangefinder_rays(m0)
  m = rc.model(rc.rig_sites(m0, pnt, vec))
  b = six_batch(64, model=m)
  rig = m.name2id('rig', 'body')
  br = rays.BatchRays(b)
  dist, gid = br.cast(tensor(b, pnt), tensor(b, vec), bodyexclude='rig')
  sensor = b.get('sensordata')
  dist, gid = dist.cpu().numpy(), gid.cpu().numpy()
  metres = np.where(gid >= 0, dist*np.linalg.norm(vec, axis=1), -1.0)
  assert sensor.shape == (B, 48) and (gid >= 0).any() and (gid < 0).any()
  np.testing.assert_allclose(metres, sensor, rtol=0, atol=1e-9)
  assert not np.array_equal(metres[0], metres[1])      # the environments differ
  # the same rays as scans in the sites' own frames: several one-ray scans share a launch
  for i in range(4):
    br.add_scan(dict(site='ray%d' % i), [[0, 0, 1.0]])
  assert br.scans[0]['bodyexclude'] == rig
  sd, sg = br.scan()
  np.testing.assert_allclose(sd.cpu().numpy()[:, :, 0], sensor[:, :4], rtol=0, atol=1e-9)
  assert np.array_equal(sg.cpu().numpy()[:, :, 0], gid[:, :4])


@pytest.mark.parametrize('batch_size', [3, 65])
def test_one_ray_per_environment_ragged_wave(batch_size):
  from dm_control_amd import rays
  b = six_batch(64, batch_size)
  m = b.model
  rs = np.random.RandomState(11)
  o, v = rc.seeded_rays(0, 512)
  pick = rs.choice(512, batch_size, replace=False)
  pnt, vec = o[pick][:, None], v[pick][:, None]
  guard = tensor(b, np.full((batch_size + 64,), 7.0))      # the lanes past B*R must write nothing
  dist, gid = rays.BatchRays(b).cast(tensor(b, pnt), tensor(b, vec), out=(guard[:batch_size].view(batch_size, 1),
                                                                          tensor(b, np.zeros((batch_size, 1))).int()))
  st = read_state(b)
  assert np.all(guard.cpu().numpy()[batch_size:] == 7.0)
  dist, gid = dist.cpu().numpy(), gid.cpu().numpy()
  hits = 0
  for e in range(batch_size):
    tw = rt.cast(m, st['geom_xpos'][e], st['geom_xmat'][e], pnt[e], vec[e])
    if tw['excluded'][0]:
      continue
    assert gid[e, 0] == tw['gid'][0], e
    assert rc.rel_error(dist[e], tw['dist'], vec[e])[0] <= rc.TOL_F64 if tw['gid'][0] >= 0 else dist[e, 0] == -1
    hits += tw['gid'][0] >= 0
  assert hits > batch_size // 3


def many_spheres_model(n=150):
  """More hittable geoms than one staging pass of the scan kernel: non-colliding world spheres around the origin, a floor,
  and a free ball so that the model has a state.  Every fifth sphere sits at the height of the scans below, alternately 3 m
  and 3.4 m out; the others hang above them, out of the scans' way but not out of the staging's."""
  az = 2*np.pi*np.arange(n)/n
  spheres = ''.join('<geom name="s%d" type="sphere" size=".05" pos="%r %r %r" contype="0" conaffinity="0"/>'
                    % (i, float((3 + 0.4*(i % 2))*np.cos(a)), float((3 + 0.4*(i % 2))*np.sin(a)), 0.5 if i % 5 == 0 else 2.5 + 0.3*(i % 3))
                    for i, a in enumerate(az))
  return mc.compile_xml('<mujoco><worldbody><geom name="floor" type="plane" size="5 5 .1"/>%s<body name="ball" pos="0 0 .8">'
                        '<freejoint/><geom name="ballg" type="sphere" size=".1"/></body></worldbody></mujoco>' % spheres)


def test_scan_second_ragged_tile_two_scans_many_geoms_and_one_environment():
  """R = 257: a second tile with one live lane; two scans in one launch; 152 geoms: three staging passes; B = 1."""
  from dm_control_amd import rays
  m = many_spheres_model()
  b = make_batch(m, 64, 1)
  b.forward()
  b.sync()
  br = rays.BatchRays(b)
  info = br.info()
  assert info['geoms'] == 152 > 2*info['scan_pass'] and info['scan_tile'] < 257
  dirs = rays.ring(257, elevations=(0.0,))
  dirs[::3] *= 1.7       # not unit length
  dirs[1::3, 2] = -0.25       # some towards the floor
  br.add_scan('world', dirs, offset=(0, 0, 0.5))
  br.add_scan(dict(body='ball'), dirs*1.5, offset=(0.02, 0, -0.3), bodyexclude=-1)
  dist, gid = br.scan()
  assert tuple(dist.shape) == (1, 2, 257)
  st = read_state(b)
  dist, gid = dist.cpu().numpy(), gid.cpu().numpy()
  assert against_twin(m, st, 0, np.tile([0, 0, 0.5], (257, 1)), dirs, dist[0, 0], gid[0, 0], 'world scan') <= rc.TOL_F64
  o, v = br.scan_rays(1, st['xpos'][0], st['xmat'][0], st['site_xpos'][0], st['site_xmat'][0], st['geom_xpos'][0], st['geom_xmat'][0])
  assert against_twin(m, st, 0, np.tile(o, (257, 1)), v, dist[0, 1], gid[0, 1], 'ball scan') <= rc.TOL_F64
  assert gid[0, 0].max() > 2*info['scan_pass'] and (gid[0, 0] >= 0).sum() > 40      # geoms of the third pass were hit
  assert gid[0, 0, 256] == rt.cast(m, st['geom_xpos'][0], st['geom_xmat'][0], [[0, 0, 0.5]], dirs[256:], edge=False)['gid'][0]
  # the cutoff's cull at staging time never changes a result: the same scan with a cutoff equals the filtered one
  cut = rays.BatchRays(b, cutoff=3.1)
  cut.add_scan('world', dirs, offset=(0, 0, 0.5))
  cd, cg = (t.cpu().numpy() for t in cut.scan())
  metres = dist[0, 0]*np.linalg.norm(dirs, axis=1)
  inside = (gid[0, 0] >= 0) & (metres <= 3.1)
  assert inside.any() and (~inside & (gid[0, 0] >= 0)).any()
  assert np.array_equal(cd[0, 0][inside], dist[0, 0][inside]) and np.array_equal(cg[0, 0][inside], gid[0, 0][inside])
  assert np.all(cd[0, 0][~inside] == -1) and np.all(cg[0, 0][~inside] == -1)


def test_bodyexclude_tensor_filters_and_camera_frame():
  import torch
  from dm_control_amd import rays
  b = six_batch(64)
  m = b.model
  ball, rig = m.name2id('ball', 'body'), m.name2id('rig', 'body')
  st = read_state(b)
  top = st['xpos'].reshape(B, -1, 3)[:, ball] + [0, 0, 0.5]
  pnt = tensor(b, np.repeat(top[:, None], 2, 1))
  br = rays.BatchRays(b)
  bex = torch.tensor([[-1, ball]] * B, dtype=torch.int32, device='cuda')
  dist, gid = br.cast(pnt, tensor(b, [0, 0, -2.0]), bodyexclude=bex)
  gid, dist = gid.cpu().numpy(), dist.cpu().numpy()
  ballg = m.name2id('ballg', 'geom')
  assert np.all(gid[:, 0] == ballg) and np.allclose(dist[:, 0], 0.2, atol=1e-9) and np.all(gid[:, 1] != ballg)
  per_env = torch.tensor([ball, -1, ball], dtype=torch.int32, device='cuda')
  g2 = br.cast(pnt, tensor(b, [0, 0, -2.0]), bodyexclude=per_env)[1].cpu().numpy()
  assert [list(r) for r in g2 == ballg] == [[False, False], [True, True], [False, False]]
  assert np.array_equal(br.cast(pnt, tensor(b, [0, 0, -2.0]), bodyexclude='ball')[1].cpu().numpy()[:, 0], gid[:, 1])
  with pytest.raises(ValueError):
    br.cast(pnt, tensor(b, [0, 0, -2.0]), bodyexclude=torch.zeros(B + 1, dtype=torch.int32))
  # the filters fixed at create time, against the twin on one environment
  o, v = rc.seeded_rays(0)
  for kw in (dict(geomgroup=(1, 1, 1, 0, 0, 0)), dict(flg_static=0), dict(cutoff=0.8)):
    d, g = rays.BatchRays(b, **{k: (bool(x) if k == 'flg_static' else x) for k, x in kw.items()}).cast(tensor(b, o), tensor(b, v))
    assert against_twin(m, st, 0, o, v, d.cpu().numpy()[0], g.cpu().numpy()[0], str(kw), **kw) <= rc.TOL_F64
  hidden = m.name2id('hidden', 'geom')
  d, g = rays.BatchRays(b).cast(tensor(b, [0, 0, 1.0]), tensor(b, [0, 0, -1.0]))
  assert np.all(g.cpu().numpy() == hidden)
  d, g = rays.BatchRays(b, geomgroup=(1, 1, 1, 0, 0, 0)).cast(tensor(b, [0, 0, 1.0]), tensor(b, [0, 0, -1.0]))
  assert np.all(g.cpu().numpy() == m.name2id('floor', 'geom'))
  # a fixed camera's frame: the ray along its optical axis (-z) is the centre pixel of a depth image
  from dm_control_amd import camera
  br.add_scan(dict(camera='eye'), [[0, 0, -1.0]])
  sd, sg = br.scan()
  img = camera.BatchCamera(b, ['eye'], 1, 1).render_all()
  assert np.array_equal(sg.cpu().numpy()[:, 0, 0], img['segmentation'].cpu().numpy()[:, 0, 0, 0, 0])
  hit = sg.cpu().numpy()[:, 0, 0] >= 0
  assert hit.any() and np.allclose(sd.cpu().numpy()[:, 0, 0][hit], img['depth'].cpu().numpy()[:, 0, 0, 0][hit], rtol=1e-9)
  assert br.skipped_geoms == []


def test_geom_size_follows_set_model_real_and_env_geoms():
  from dm_control_amd import rays
  b = six_batch(64)
  m = b.model
  br = rays.BatchRays(b)
  br.add_scan('world', rays.ring(96, elevations=(-0.9,)), offset=(0.1, 0.0, 0.9))
  o, v = rc.seeded_rays(0)
  pnt, vec = tensor(b, o), tensor(b, v)
  box, cyl = m.name2id('box', 'geom'), m.name2id('cyl', 'geom')
  g0 = br.cast(pnt, vec)[1].cpu().numpy()
  size = np.array(m.geom_size, dtype=np.float64)
  size[box] *= 1.5
  b.set_model_real('geom_size', size)
  b.forward()
  b.sync()
  d1, g1 = (t.cpu().numpy() for t in br.cast(pnt, vec))
  assert (g1 == box).sum() > (g0 == box).sum() > 0
  st = read_state(b)
  for e in (0, B - 1):
    assert against_twin(m, st, e, o, v, d1[e], g1[e], 'grown box', geom_size=size) <= rc.TOL_F64
  # per-environment geoms: the cylinder shrinks in environment 2 only
  s1 = [t.cpu().numpy() for t in br.scan()]
  b.set_env_geoms(['cyl'])
  b.set_env_geom('cyl', size=np.where(np.arange(B)[:, None] == 2, 0.5, 1.0)*size[cyl])
  b.forward()
  b.sync()
  d2, g2 = (t.cpu().numpy() for t in br.cast(pnt, vec))
  s2 = [t.cpu().numpy() for t in br.scan()]
  for e in range(B):
    n1, n2 = (g1[e] == cyl).sum(), (g2[e] == cyl).sum()
    assert (0 < n2 < n1) if e == 2 else (n2 == n1 > 0), (e, n1, n2)
    same = np.array_equal(d1[e], d2[e]) and np.array_equal(g1[e], g2[e]) and all(np.array_equal(x[e], y[e]) for x, y in zip(s1, s2))
    assert same == (e != 2), e      # only the changed environment's results change
  small = size.copy()
  small[cyl] *= 0.5
  st = read_state(b)
  assert against_twin(m, st, 2, o, v, d2[2], g2[2], 'shrunk cylinder', geom_size=small) <= rc.TOL_F64
  po, pv = br.scan_rays(0, *[st[k][2] for k in ('xpos', 'xmat', 'site_xpos', 'site_xmat', 'geom_xpos', 'geom_xmat')])
  assert against_twin(m, st, 2, np.tile(po, (96, 1)), pv, s2[0][2, 0], s2[1][2, 0], 'shrunk cylinder scan', geom_size=small) <= rc.TOL_F64


def test_stale_poses_are_refused():
  from dm_control_amd import _native, rays
  from dm_control_amd.batch import OUT, OUT_ALL
  m = rc.model()
  fresh = make_batch(m, 32)      # no launch yet: nothing to cast against
  br = rays.BatchRays(fresh)
  pnt, vec = tensor(fresh, [0, 0, 1.0]), tensor(fresh, [0, 0, -1.0])
  with pytest.raises(_native.NativeError, match='output mask'):
    br.cast(pnt, vec)
  fresh.forward()
  br.cast(pnt, vec)
  b = six_batch(32)
  br = rays.BatchRays(b)
  br.add_scan(dict(body='ball'), rays.ring(8))
  assert br.output_mask == OUT['geom'] | OUT['xpos'] | OUT['xmat']
  b.set_output_mask(OUT_ALL & ~OUT['geom'])
  with pytest.raises(_native.NativeError, match='output mask'):
    br.cast(pnt, vec)
  b.set_output_mask(OUT['geom'])      # a body frame reads xpos / xmat too
  br.cast(pnt, vec)
  with pytest.raises(_native.NativeError, match='output mask'):
    br.scan()
  b.set_output_mask(br.output_mask)
  br.scan()
  # the mask the LAST LAUNCH ran with counts too
  b.set_output_mask(OUT['xpos'] | OUT['xmat'])
  b.step()
  b.set_output_mask(OUT_ALL)
  with pytest.raises(_native.NativeError, match='output mask'):
    br.cast(pnt, vec)
  b.forward()
  br.cast(pnt, vec)
  with pytest.raises(ValueError, match='same number of directions'):
    br.add_scan('world', rays.ring(9))
  with pytest.raises(ValueError, match='no scan'):
    rays.BatchRays(b).scan()


def test_graph_replay_and_normals_leave_the_other_outputs_alone():
  import torch
  from dm_control_amd import rays
  b = six_batch(32)
  m = b.model
  br = rays.BatchRays(b)
  br.add_scan(dict(body='ball'), rc.ring_dirs())
  o, v = rc.seeded_rays(1)
  pnt, vec = tensor(b, o), tensor(b, v)
  plain = br.cast(pnt, vec)
  with_n = br.cast(pnt, vec, normals=True)
  assert torch.equal(plain[0], with_n[0]) and torch.equal(plain[1], with_n[1])
  hit = with_n[1] >= 0
  assert torch.allclose(with_n[2][hit].norm(dim=-1), torch.ones((), device='cuda'), atol=1e-5) and bool((with_n[2][~hit] == 0).all())
  sp, sn = br.scan(), br.scan(normals=True)
  assert torch.equal(sp[0], sn[0]) and torch.equal(sp[1], sn[1])
  # a forward, a cast and a scan recorded into one graph on one stream
  out_c = [torch.zeros_like(t) for t in plain]
  out_s = [torch.zeros_like(t) for t in sp]
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    b.forward(stream=torch.cuda.current_stream().cuda_stream)
    br.cast(pnt, vec, out=out_c)
    br.scan(out=out_s)
  q = np.stack([rc.state_qpos(m, (e + 1) % rc.NSTATE) for e in range(B)])      # the state moves; the graph is replayed
  b.set('qpos', q)
  for t in out_c + out_s:
    t.zero_()
  graph.replay()
  torch.cuda.synchronize()
  b.forward()
  eager_c, eager_s = br.cast(pnt, vec), br.scan()
  assert not torch.equal(eager_c[0], plain[0]) and not torch.equal(eager_s[0], sp[0])      # the state did move
  for x, y in zip(out_c + out_s, eager_c + eager_s):
    assert torch.equal(x, y)


def test_lidar_wrap_fused_cheetah():
  import torch
  from dm_control_amd import rays
  from dm_control_amd.suite import fused_env, lidar
  env = fused_env.make('cheetah', 'run', 4)
  dirs = rays.ring(16, elevations=(-0.5, -0.2))
  lenv = lidar.wrap(env, dict(body='torso'), dirs, lidar_only=True, cutoff=6.0)
  obs = lenv.reset()
  assert tuple(obs.shape) == (4, 32) and obs.dtype == env.dtype and obs.device.type == 'cuda'
  act = torch.zeros((4, env.model.nu), dtype=env.dtype, device=env.device)
  for _ in range(3):
    act.uniform_(-1, 1)
    obs, reward, done = lenv.step(act)
  assert torch.equal(obs, lenv.scan()) and reward.shape == (4,)
  b = lenv.rays.batch
  st = read_state(b)
  m = b.model
  torso = m.name2id('torso', 'body')
  assert lenv.rays.scans[0]['bodyexclude'] == torso      # the agent's own body is not in its scan
  obs = obs.cpu().numpy()
  gid = lenv.rays.scan()[1].cpu().numpy()
  assert (obs >= 0).any() and not np.any(np.isin(gid, np.nonzero(np.asarray(m.geom_bodyid) == torso)[0]))
  for e in (0, 3):
    o, v = lenv.rays.scan_rays(0, *[st[k][e] for k in STATE[2:] + STATE[:2]])
    err = against_twin(m, st, e, np.tile(o, (32, 1)), v, obs[e].astype(np.float64), gid[e, 0], 'cheetah lidar', bodyexclude=torso, cutoff=6.0)
    print('cheetah lidar env %d: %.4g' % (e, err))
    assert err <= rc.TOL_F32_ONE_STEP
  # tanh squashing on the device: misses read 1, hits tanh(dist / cutoff)
  squashed = lidar.wrap(env, dict(body='torso'), dirs, cutoff=6.0, scale='tanh')
  o2 = squashed.step(act)[0]
  raw = squashed.rays.scan()[0][:, 0]
  assert set(o2) == {'state', 'lidar'} and tuple(o2['lidar'].shape) == (4, 32)
  assert torch.equal(o2['lidar'], torch.where(raw < 0, torch.ones_like(raw), torch.tanh(raw / 6.0)))
  assert bool((raw < 0).any()) and float(o2['lidar'].max()) == 1.0 and float(o2['lidar'].min()) > 0


def test_lidar_wrap_composer_soccer_and_capture_rule():
  import torch
  from dm_control_amd import composer, rays
  from dm_control_amd.suite import lidar
  env = composer.make('soccer_2v2', 2)
  dirs = rays.ring(24, elevations=(0.0, -0.3), fov=np.pi)
  dirs = np.stack([dirs[:, 1], dirs[:, 2], -dirs[:, 0]], 1)      # a fan about the camera's optical axis, -z
  lenv = lidar.wrap(env, dict(camera='home0/egocentric'), dirs, lidar_only=True)
  ts = lenv.reset()
  scan = ts.observation['lidar']
  assert set(ts.observation) == {'lidar'} and tuple(scan.shape) == (2, 48) and scan.device.type == 'cuda'
  spec = env.action_spec() if hasattr(env, 'action_spec') else None
  nu = int(np.prod(spec.shape[1:])) if spec is not None else lenv.rays.model.nu
  for _ in range(2):
    ts = lenv.step(torch.zeros((2, nu), device=scan.device).uniform_(-1, 1))
  scan = ts.observation['lidar']
  assert torch.equal(scan, lenv.scan())
  b, m = lenv.rays.batch, lenv.rays.model
  st = read_state(b)
  own = lenv.rays.scans[0]['bodyexclude']
  assert own == lenv.rays.scans[0]['frame']['body'] >= 1
  gid = lenv.rays.scan()[1].cpu().numpy()
  assert not np.any(np.isin(gid, np.nonzero(np.asarray(m.geom_bodyid) == own)[0])) and (gid >= 0).any()
  tol = rc.TOL_F64 if b.precision == 64 else rc.TOL_F32_ONE_STEP
  for e in range(2):
    o, v = lenv.rays.scan_rays(0, *[st[k][e] for k in STATE[2:] + STATE[:2]])
    err = against_twin(m, st, e, np.tile(o, (48, 1)), v, scan[e].cpu().numpy().astype(np.float64), gid[e, 0], 'soccer lidar', bodyexclude=own)
    print('soccer lidar env %d (fp%d): %.4g' % (e, b.precision, err))
    assert err <= tol

  class Captured:      # an environment that holds a recorded graph and cannot re-record it by itself
    _graph = object()

    def __init__(self, physics):
      self.physics = physics
  with pytest.raises(ValueError, match='before recording'):
    lidar.wrap(Captured(six_batch(32)), 'world', rays.ring(4))


def test_mj_ray_on_a_hip_physics_equals_the_cpu_tier():
  from dm_control_amd import mujoco_api as mj
  from oracle.oracle import OraclePhysics
  m = rc.model()
  model = mj.MjModel.from_xml_string(cs.six_primitive_xml())
  data = mj.MjData(model)
  data.qpos[:] = rc.state_qpos(m, 1)
  mj.mj_forward(model, data)
  p = OraclePhysics(m)
  p.qpos[:] = rc.state_qpos(m, 1)
  p.forward()
  o, v = rc.seeded_rays(1, 24)
  tw = rt.cast(m, p.geom_xpos, p.geom_xmat, o, v)      # the CPU tier's value: the twin on the oracle's poses
  geomid = np.zeros(1, dtype=np.int32)
  checked = 0
  for i in np.nonzero(~tw['excluded'])[0]:
    x = mj.mj_ray(model, data, o[i], v[i], None, 1, -1, geomid)
    assert geomid[0] == tw['gid'][i] and abs(x - tw['dist'][i]) <= 1e-9*max(1.0, abs(tw['dist'][i]))
    checked += 1
  assert checked >= 20

"""Ray-cast cameras on the GPU: the render kernel against the numpy twin (tests/camera_twin.py), which is always fed the
device's own poses read back with `batch.get` -- only the camera is under test.

Measured on an MI355X over the scenes below (max |d depth| / max(1, depth) on non-excluded pixels, against the twin):
  fp64 batch: 1.0e-13 (six primitives), 1.7e-13 (soccer); bound: the project's fp64 tolerance, 1e-9 relative
  fp32 batch: 1.303e-6 (six primitives, the cylinder), 7.5e-7 (soccer, a pitch plane 46 m away); bound 4 x the maximum
"""
import numpy as np
import pytest

import camera_scenes as cs
import camera_twin as twin
from dm_control_amd import mjcf_compiler as mc

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-9
EDGE_CAP = 0.03
# fp32: measured maximum of |d depth| / max(1, depth) against the twin over the two scenes (all cameras, B = 8); the bound
# is 4 x that, to leave room for other states.  See DESIGN.md "Ray-cast cameras".
F32_DEPTH_MEASURED = 1.303e-6      # six-primitive scene, the cylinder `cyl` seen by `targetcom`; soccer: 7.544e-7; below TOL_F32_ONE_STEP (5e-5)
F32_DEPTH_TOL = 4 * F32_DEPTH_MEASURED
STATE = ('geom_xpos', 'geom_xmat', 'xpos', 'xmat', 'subtree_com')
B = 8
HW = cs.SIX_HW


def _batch(xml, precision, **kw):
  from dm_control_amd.batch import BatchedPhysics
  return BatchedPhysics(mc.compile_xml(xml), B, precision=precision, **kw)


def six_batch(precision):
  """The six-primitive scene, a different state per environment, after some steps."""
  b = _batch(cs.six_primitive_xml(), precision)
  m = b.model
  q = np.tile(m.qpos0, (B, 1))
  k = np.arange(B)
  q[:, 0] += 0.08*k - 0.2
  q[:, 1] -= 0.05*k
  q[:, 2] += 0.1*k
  q[:, 7] = 0.25*k - 0.8
  b.set('qpos', q)
  b.step(12)
  b.sync()
  return b


def soccer_batch(precision):
  b = _batch(cs.soccer_xml(), precision, nconmax=24)
  rng = np.random.RandomState(5)
  b.set('ctrl', rng.uniform(-1, 1, (B, b.model.nu)))
  b.step(25)
  b.sync()
  return b


def read_state(b):
  return {k: b.get(k) for k in STATE}


def compare(b, cam, names, prec, label, hw=HW):
  """Renders everything in one launch and compares it with the twin; returns the worst relative depth error."""
  m = b.model
  out = cam.render_all()
  st = read_state(b)
  depth, seg, rgb = out['depth'].cpu().numpy(), out['segmentation'].cpu().numpy(), out['rgb'].cpu().numpy()
  assert depth.dtype == (np.float64 if prec == 64 else np.float32) and seg.dtype == np.int32 and rgb.dtype == np.uint8
  H, W = hw
  assert depth.shape == (B, len(names), H, W) and seg.shape == (B, len(names), H, W, 2) and rgb.shape == (B, len(names), H, W, 3)
  # each single-output render is the same image
  assert np.array_equal(cam.render().cpu().numpy(), rgb)
  assert np.array_equal(cam.render(depth=True).cpu().numpy(), depth)
  assert np.array_equal(cam.render(segmentation=True).cpu().numpy(), seg)
  # the per-tile cull only drops geoms no ray of the tile can hit: the images without it are the same bits
  cam.set_tuning(cull=False)
  plain = cam.render_all()
  cam.set_tuning(cull=True)
  assert np.array_equal(plain['depth'].cpu().numpy(), depth) and np.array_equal(plain['segmentation'].cpu().numpy(), seg)
  assert np.array_equal(plain['rgb'].cpu().numpy(), rgb)
  # the tuning study's path without the pre-transform is the same camera (other association of the same arithmetic)
  cam.set_tuning(pretransform=False)
  world = cam.render_all()
  cam.set_tuning()
  wd, ws = world['depth'].cpu().numpy(), world['segmentation'].cpu().numpy()
  agree = ws[..., 0] == seg[..., 0]
  assert agree.mean() > 0.999
  fin = agree & (seg[..., 0] >= 0)
  assert np.abs(wd[fin] - depth[fin]).max() <= (1e-9 if prec == 64 else 2e-5) * max(1.0, depth[fin].max())
  worst, worst_at = 0.0, None
  for e in range(B):
    for k, (d, g, c, ex) in enumerate(cs.twin_images(m, cam.cameras, H, W, st, e)):
      frac = ex.mean()
      print('%s fp%d env %d cam %d: excluded %.4f' % (label, prec, e, k, frac))
      assert frac <= EDGE_CAP, (label, e, k, frac)
      keep = ~ex
      assert np.array_equal(seg[e, k, ..., 0][keep], g[keep]), (label, e, k)
      assert np.array_equal(seg[e, k, ..., 1][keep], np.where(g[keep] >= 0, 5, -1)), (label, e, k)
      hit = keep & (g >= 0)
      assert np.all(np.isinf(depth[e, k][keep & (g < 0)]))
      err = np.abs(depth[e, k][hit] - d[hit]) / np.maximum(1, d[hit])
      if err.size and err.max() > worst:
        gi = g[hit][err.argmax()]
        worst, worst_at = float(err.max()), (e, k, int(gi), int(m.geom_type[gi]))
      assert np.abs(rgb[e, k][keep].astype(int) - c[keep].astype(int)).max() <= 1, (label, e, k)
  print('%s fp%d: max |d depth| / max(1, depth) = %.4g at (env, cam, geom, type) %s' % (label, prec, worst, worst_at))
  return worst


@pytest.fixture(scope='module')
def camera_lib():
  from dm_control_amd import camera
  return camera


def test_fp64_six_primitives_all_modes(camera_lib):
  b = six_batch(64)
  cam = camera_lib.BatchCamera(b, list(cs.SIX_CAMERAS), *HW)
  st = read_state(b)
  assert np.abs(st['geom_xpos'][0] - st['geom_xpos'][B - 1]).max() > 0.1      # the environments differ
  assert compare(b, cam, cs.SIX_CAMERAS, 64, 'six') < TOL_F64
  # matrices(): the targetbody camera centres its target in every environment
  M = cam.matrices()
  ball = b.model.name2id('ball', 'body')
  for e in range(B):
    x, y, w = M[e, 3] @ np.append(st['xpos'][e].reshape(-1, 3)[ball], 1.0)
    np.testing.assert_allclose([x/w, y/w], [(HW[1] - 1)/2, (HW[0] - 1)/2], atol=1e-6)


def test_fp64_soccer_all_modes(camera_lib):
  b = soccer_batch(64)
  cam = camera_lib.BatchCamera(b, list(cs.SOCCER_CAMERAS), *cs.SOCCER_HW)
  assert sorted(set(c['mode'] for c in cam.cameras)) == [0, 1, 2, 3, 4]
  assert compare(b, cam, cs.SOCCER_CAMERAS, 64, 'soccer', cs.SOCCER_HW) < TOL_F64


def test_fp32_both_scenes(camera_lib):
  worst = 0.0
  for label, make, names, hw in (('six', six_batch, cs.SIX_CAMERAS, cs.SIX_HW), ('soccer', soccer_batch, cs.SOCCER_CAMERAS, cs.SOCCER_HW)):
    b = make(32)
    cam = camera_lib.BatchCamera(b, list(names), *hw)
    worst = max(worst, compare(b, cam, names, 32, label, hw))
  print('fp32: max |d depth| / max(1, depth) over both scenes = %.4g' % worst)
  assert worst < F32_DEPTH_TOL, worst


def test_only_the_changed_environments_image_changes(camera_lib):
  b = six_batch(64)
  cam = camera_lib.BatchCamera(b, ['eye', 'track'], *HW)
  before = cam.render_all()
  before = {k: v.cpu().numpy() for k, v in before.items()}
  q = b.get('qpos')
  q[3, :3] += [0.2, 0.1, 0.3]
  b.set('qpos', q)
  b.forward()
  after = {k: v.cpu().numpy() for k, v in cam.render_all().items()}
  for k in before:
    same = [np.array_equal(before[k][e], after[k][e]) for e in range(B)]
    assert same == [e != 3 for e in range(B)], (k, same)


def test_geom_size_follows_set_model_real_and_env_geoms(camera_lib):
  b = six_batch(64)
  m = b.model
  cam = camera_lib.BatchCamera(b, ['eye'], *HW)
  H, W = HW
  box, cyl = m.name2id('box', 'geom'), m.name2id('cyl', 'geom')
  seg0 = cam.render(segmentation=True).cpu().numpy()[..., 0]
  size = np.array(m.geom_size, dtype=np.float64)
  size[box] *= 1.5
  b.set_model_real('geom_size', size)
  b.forward()
  b.sync()
  seg1 = cam.render(segmentation=True).cpu().numpy()[..., 0]
  assert (seg1 == box).sum() > 1.5*(seg0 == box).sum() > 0
  st = read_state(b)
  cams = cam.cameras
  for e in (0, B - 1):
    d, g, _, ex = cs.twin_images(m, cams, H, W, st, e, geom_size=size)[0]
    assert ex.mean() <= EDGE_CAP, ex.mean()
    assert np.array_equal(seg1[e, 0][~ex], g[~ex])
  # per-environment geoms: the cylinder shrinks in environment 2 only
  b.set_env_geoms(['cyl'])
  b.set_env_geom('cyl', size=np.where(np.arange(B)[:, None] == 2, 0.5, 1.0)*size[cyl])
  b.forward()
  b.sync()
  seg2 = cam.render(segmentation=True).cpu().numpy()[..., 0]
  for e in range(B):
    n1, n2 = (seg1[e] == cyl).sum(), (seg2[e] == cyl).sum()
    assert (n2 < 0.6*n1) if e == 2 else (n2 == n1), (e, n1, n2)
  st = read_state(b)
  small = size.copy()
  small[cyl] *= 0.5
  d, g, _, ex = cs.twin_images(m, cams, H, W, st, 2, geom_size=small)[0]
  assert ex.mean() <= EDGE_CAP, ex.mean()
  assert np.array_equal(seg2[2, 0][~ex], g[~ex])


def test_recolouring_changes_rgb_only(camera_lib):
  b = six_batch(32)
  m = b.model
  cam = camera_lib.BatchCamera(b, ['eye'], *HW)
  a = {k: v.cpu().numpy() for k, v in cam.render_all().items()}
  box = m.name2id('box', 'geom')
  old = m.geom_rgba[box].copy()
  try:
    m.geom_rgba[box] = [0.1, 0.9, 0.1, 1]
    c = {k: v.cpu().numpy() for k, v in cam.render_all().items()}
  finally:
    m.geom_rgba[box] = old
  assert np.array_equal(a['depth'], c['depth']) and np.array_equal(a['segmentation'], c['segmentation'])
  changed = np.any(a['rgb'] != c['rgb'], axis=-1)
  assert changed.any() and np.array_equal(changed, a['segmentation'][..., 0] == box)
  # the material's colour is drawn where the geom's own is the default grey
  painted = m.name2id('painted', 'geom')
  px = a['rgb'][a['segmentation'][..., 0] == painted]
  assert px.size and np.all(px[:, 0] > 3*px[:, 1])


def test_near_far_groups_and_alpha(camera_lib):
  b = six_batch(64)
  m = b.model
  base = camera_lib.BatchCamera(b, ['eye'], *HW)
  d0 = base.render(depth=True).cpu().numpy()
  s0 = base.render(segmentation=True).cpu().numpy()[..., 0]
  assert m.name2id('ghost', 'geom') not in s0 and m.name2id('hidden', 'geom') not in s0
  clip = camera_lib.BatchCamera(b, ['eye'], *HW, near=1.9, far=2.6)
  d1 = clip.render(depth=True).cpu().numpy()
  s1 = clip.render(segmentation=True).cpu().numpy()[..., 0]
  assert (d0 < 1.9).any() and np.all(d1[s1 >= 0] >= 1.9) and np.all(d1[s1 >= 0] <= 2.6) and np.all(d1[s1 < 0] == 2.6)
  inside = (d0 >= 1.9) & (d0 <= 2.6)
  assert np.array_equal(d1[inside], d0[inside]) and np.array_equal(s1[inside], s0[inside])
  allg = camera_lib.BatchCamera(b, ['eye'], *HW, geom_groups=(0, 1, 2, 3))
  assert m.name2id('hidden', 'geom') in allg.render(segmentation=True).cpu().numpy()[..., 0]
  bg = camera_lib.BatchCamera(b, ['eye'], *HW, background=(0.2, 0.4, 1.0))
  rgb = bg.render().cpu().numpy()
  assert np.all(rgb[s0 < 0] == [51, 102, 255]) and (s0 < 0).any()


def test_errors(camera_lib):
  from dm_control_amd import _native
  from dm_control_amd.batch import OUT, OUT_ALL
  b = six_batch(32)
  cam = camera_lib.BatchCamera(b, ['eye'], *HW)
  with pytest.raises(ValueError):
    cam.render(depth=True, segmentation=True)
  b.set_output_mask(OUT_ALL & ~OUT['geom'])
  with pytest.raises(_native.NativeError, match='output mask'):
    cam.render()
  b.set_output_mask(OUT['geom'] | OUT['xpos'])      # a fixed camera reads xmat too
  with pytest.raises(_native.NativeError, match='output mask'):
    cam.render()
  b.set_output_mask(OUT['geom'] | OUT['xpos'] | OUT['xmat'])
  cam.render()
  # the mask the LAST LAUNCH ran with counts too: poses a step did not write are stale even after the mask is widened
  b.set_output_mask(OUT['xpos'] | OUT['xmat'])
  b.step()
  b.set_output_mask(OUT_ALL)
  with pytest.raises(_native.NativeError, match='output mask'):
    cam.render()
  b.forward()
  cam.render()
  fresh = six_batch.__globals__['_batch'](cs.six_primitive_xml(), 32)      # no launch yet: nothing to draw
  with pytest.raises(_native.NativeError, match='output mask'):
    camera_lib.BatchCamera(fresh, ['eye'], *HW).render()
  from dm_control_amd import physics as physics_lib
  p = physics_lib.Physics.from_xml_string(cs.six_primitive_xml(), batch_size=2)
  with pytest.raises(NotImplementedError):      # the new capability lives under new names only
    p.render()
  p.free()


def test_pixels_wrap_fused_cheetah(camera_lib):
  import torch
  from dm_control_amd.suite import fused_env, pixels
  env = fused_env.make('cheetah', 'run', 64)
  spec = dict(body='torso', pos=(0, -3, 0.5), xyaxes=(1, 0, 0, 0, 0, 1), mode='trackcom', fovy=45)
  penv = pixels.wrap(env, [spec])
  obs = penv.reset()
  assert obs.shape == (64, 1, 84, 84, 3) and obs.dtype == torch.uint8 and obs.device.type == 'cuda'
  act = torch.zeros((64, env.model.nu), dtype=env.dtype, device=env.device)
  for _ in range(5):
    act.uniform_(-1, 1)
    obs, reward, done = penv.step(act)
  direct = penv.camera.render()
  assert torch.equal(obs, direct)
  assert reward.shape == (64,) and obs.float().std() > 1      # an image with something in it
  seg = penv.camera.render(segmentation=True)
  assert (seg[..., 0] >= 0).float().mean() > 0.05      # the cheetah and the floor are in view
  # the image is the twin's, from the device's own poses
  b = penv.camera.batch
  torch.cuda.synchronize()
  st = read_state(b)
  d, g, c, ex = cs.twin_images(b.model, penv.camera.cameras, 84, 84, st, 7)[0]
  assert ex.mean() <= EDGE_CAP, ex.mean()
  assert np.array_equal(seg[7, 0, ..., 0].cpu().numpy()[~ex], g[~ex])
  assert np.abs(obs[7, 0].cpu().numpy().astype(int)[~ex] - c[~ex].astype(int)).max() <= 1
  # over an episode restart the first observation of the new episode shows the new state
  env.restart()      # every environment starts a new episode with the next step
  obs2, _, _ = penv.step(act)
  assert bool(env.first.all())
  torch.cuda.synchronize()
  st2 = read_state(b)
  d2, g2, c2, ex2 = cs.twin_images(b.model, penv.camera.cameras, 84, 84, st2, 7)[0]
  assert ex2.mean() <= EDGE_CAP, ex2.mean()
  assert np.abs(obs2[7, 0].cpu().numpy().astype(int)[~ex2] - c2[~ex2].astype(int)).max() <= 1
  dkind = pixels.wrap(env, [spec], 32, 48, kind='depth', pixels_only=False)
  o = dkind.step(act)[0]
  assert o['pixels'].shape == (64, 1, 32, 48) and o['pixels'].dtype == torch.float32 and o['state'].shape[0] == 64


def test_pixels_wrap_torch_env_and_device_env(camera_lib):
  import torch
  from dm_control_amd.suite import device_env, pixels, torch_env
  spec = dict(body='torso', pos=(0, -3, 0.5), xyaxes=(1, 0, 0, 0, 0, 1), mode='trackcom', fovy=45)
  for make in (torch_env.make, device_env.make):
    env = make('cheetah', 'run', 16)
    penv = pixels.wrap(env, [spec], 32, 48)
    penv.reset()
    nu = penv.camera.model.nu
    for _ in range(3):      # (the second and third step replay the environment's recorded graph, if it records one)
      out = penv.step(torch.zeros((16, nu), device='cuda').uniform_(-1, 1))
    obs = out[0] if isinstance(out, tuple) else out.observation['pixels'] if hasattr(out, 'observation') else out
    assert obs.shape == (16, 1, 32, 48, 3) and obs.dtype == torch.uint8 and obs.device.type == 'cuda'
    assert torch.equal(obs, penv.camera.render())
    seg = penv.camera.render(segmentation=True)[..., 0]
    assert (seg >= 0).float().mean() > 0.05


def test_wrapping_after_a_composer_graph_capture_is_refused(camera_lib):
  from dm_control_amd.suite import pixels

  class Captured:      # an environment that holds a recorded graph and cannot re-record it by itself
    _graph = object()

    def __init__(self, physics):
      self.physics = physics
  with pytest.raises(ValueError, match='before recording'):
    pixels.wrap(Captured(six_batch(32)), ['eye'], 16, 16)


def test_pixels_wrap_composer_soccer(camera_lib):
  import torch
  from dm_control_amd import composer
  from dm_control_amd.suite import pixels
  env = composer.make('soccer_2v2', 8)
  penv = pixels.wrap(env, list(cs.SOCCER_EGOCENTRIC), 64, 64)
  ts = penv.reset()
  img = ts.observation['pixels']
  assert set(ts.observation) == {'pixels'}
  assert img.shape == (8, 4, 64, 64, 3) and img.dtype == torch.uint8 and img.device.type == 'cuda'
  spec = env.action_spec() if hasattr(env, 'action_spec') else None
  nu = int(np.prod(spec.shape[1:])) if spec is not None else penv.camera.model.nu
  for _ in range(3):
    ts = penv.step(torch.zeros((8, nu), device=img.device).uniform_(-1, 1))
  assert torch.equal(ts.observation['pixels'], penv.camera.render())
  assert ts.observation['pixels'].float().std() > 1

"""Ray-cast camera textures on the GPU: the render kernel's textured instantiations against the fp64 numpy twin
(tests/camera_texture_twin.py), which is always fed the device's own poses read back with `batch.get`; exclusions come
from the twin alone, never from the device's output.  RGB agrees within one level on non-excluded pixels, and the excluded
share of every image is at most 3 %."""
import numpy as np
import pytest

import camera_scenes as cs
import camera_texture_scenes as ts
from dm_control_amd import mjcf_compiler as mc

pytestmark = pytest.mark.gpu

EDGE_CAP = 0.03
B = 3
HW = ts.HW


@pytest.fixture(scope='module')
def camera_lib():
  from dm_control_amd import camera
  return camera


def scene_batch(precision, case=ts.PLANE_CASES[0], xml=None, **kw):
  from dm_control_amd.batch import BatchedPhysics
  b = BatchedPhysics(mc.compile_xml(xml or ts.textured_xml(*case)), B, precision=precision, **kw)
  b.set('qpos', ts.env_qpos(b.model, B))
  b.step(ts.NSTEP)
  b.sync()
  return b


def read_state(b):
  return {k: b.get(k) for k in ts.STATE}


def images(cam):
  return {k: v.cpu().numpy() for k, v in cam.render_all().items()}


_twin_cache = {}


def twin_for(b, cam, texture_filter, tag):
  """The twin's images of every (environment, camera), computed once per (scene, precision, filter) and left unchanged."""
  key = (tag, texture_filter)
  if key not in _twin_cache:
    st = read_state(b)
    _twin_cache[key] = [ts.twin_images(b.model, cam.cameras, cam.height, cam.width, st, e, cam.materials, cam.sky, texture_filter)
                        for e in range(b.batch_size)]
  return _twin_cache[key]


def compare(b, cam, texture_filter, tag, out=None):
  out = out or images(cam)
  for e, per_cam in enumerate(twin_for(b, cam, texture_filter, tag)):
    for k, (d, g, rgb, key, ex) in enumerate(per_cam):
      print('%s %s env %d cam %d: excluded %.4f' % (tag, texture_filter, e, k, ex.mean()))
      assert ex.mean() <= EDGE_CAP, (tag, e, k, ex.mean())
      keep = ~ex
      assert np.array_equal(out['segmentation'][e, k, ..., 0][keep], g[keep]), (tag, e, k)
      diff = np.abs(out['rgb'][e, k][keep].astype(int) - rgb[keep].astype(int))
      assert diff.max() <= 1, (tag, texture_filter, e, k, int(diff.max()))
  return out


def assert_geometry_is_the_untextured_one(camera_lib, b, cam, out):
  plain = images(camera_lib.BatchCamera(b, list(ts.CAMERAS), cam.height, cam.width))
  assert np.array_equal(plain['depth'], out['depth']) and np.array_equal(plain['segmentation'], out['segmentation'])
  assert not np.array_equal(plain['rgb'], out['rgb'])
  return plain


@pytest.mark.parametrize('case', ts.PLANE_CASES)
def test_fp64_batch_nearest(camera_lib, case):
  b = scene_batch(64, case)
  st = read_state(b)
  assert np.abs(st['geom_xpos'][0] - st['geom_xpos'][B - 1]).max() > 0.1      # the environments differ
  cam = camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW, textures=True)
  assert cam.untextured == [] and cam.sky['builtin'] == 'gradient'
  out = compare(b, cam, 'nearest', ('scene64', case))
  assert_geometry_is_the_untextured_one(camera_lib, b, cam, out)
  # an image of one kind is the same image
  assert np.array_equal(cam.render().cpu().numpy(), out['rgb'])
  # every texture of the scene shows: the image holds the colours of both checker fields and of the mark
  assert len(np.unique(out['rgb'].reshape(-1, 3), axis=0)) > 50


@pytest.mark.parametrize('case', ts.PLANE_CASES)
def test_fp32_batch_nearest(camera_lib, case):
  b = scene_batch(32, case)
  cam = camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW, textures=True)
  out = compare(b, cam, 'nearest', ('scene32', case))
  assert_geometry_is_the_untextured_one(camera_lib, b, cam, out)


@pytest.mark.parametrize('prec', [64, 32])
def test_box_filter(camera_lib, prec):
  for case in ts.PLANE_CASES:
    b = scene_batch(prec, case)
    cam = camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW, textures=True, texture_filter='box')
    out = compare(b, cam, 'box', ('scene%d' % prec, case))
    near = images(camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW, textures=True))
    assert np.array_equal(near['depth'], out['depth']) and not np.array_equal(near['rgb'], out['rgb'])
    # the filter touches 2d textures on planes only
    floor = b.model.name2id('floor', 'geom')
    other = out['segmentation'][..., 0] != floor
    assert np.array_equal(near['rgb'][other], out['rgb'][other])


@pytest.mark.parametrize('prec', [64, 32])
def test_tuning_switches_draw_the_same_textured_image(camera_lib, prec):
  b = scene_batch(prec)
  for filt in camera_lib.FILTERS:
    cam = camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW, textures=True, texture_filter=filt)
    out = images(cam)
    cam.set_tuning(cull=False)
    plain = images(cam)
    cam.set_tuning(cull=True)
    for k in out:      # the cull only drops geoms no ray of the tile can hit: the same bits
      assert np.array_equal(plain[k], out[k]), (filt, k)
    cam.set_tuning(pretransform=False)
    world = images(cam)
    cam.set_tuning()
    # the agreement criterion of the untextured camera (tests/test_gpu_camera.py compare): the same hits but for a sliver, the same
    # depth to rounding -- and, where the hits agree and the twin does not exclude the pixel, the same colour within one level
    seg, depth = out['segmentation'][..., 0], out['depth']
    agree = world['segmentation'][..., 0] == seg
    assert agree.mean() > 0.999
    fin = agree & (seg >= 0)
    assert np.abs(world['depth'][fin] - depth[fin]).max() <= (1e-9 if prec == 64 else 2e-5) * max(1.0, depth[fin].max())
    ex = np.array([[c[4] for c in per_cam] for per_cam in twin_for(b, cam, filt, ('scene%d' % prec, ts.PLANE_CASES[0]))])
    ok = agree & ~ex
    assert np.abs(world['rgb'][ok].astype(int) - out['rgb'][ok].astype(int)).max() <= 1


def test_off_is_off(camera_lib):
  for prec in (64, 32):
    b = scene_batch(prec)
    default = images(camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW))
    off = images(camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW, textures=False, texture_filter='box'))
    cleared_cam = camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW)
    cleared_cam.set_materials({'floor': camera_lib.SUITE_GRID, 'box': dict(type='cube', builtin='flat', width=2, rgba=(1, 0, 0, 1))},
                              camera_lib.SUITE_SKYBOX, 'box')
    on = images(cleared_cam)
    cleared_cam.clear_materials()
    cleared = images(cleared_cam)
    for k in default:
      assert np.array_equal(default[k], off[k]) and np.array_equal(default[k], cleared[k]), (prec, k)
    assert not np.array_equal(on['rgb'], default['rgb']) and np.array_equal(on['depth'], default['depth'])
    # flat colours of the model: the untextured image is the untextured twin's
    st = read_state(b)
    for e in range(B):
      for k, (d, g, c, ex) in enumerate(cs.twin_images(b.model, cleared_cam.cameras, *HW, st, e)):
        assert np.abs(default['rgb'][e, k][~ex].astype(int) - c[~ex].astype(int)).max() <= 1
    # a record's own rgba colours a default-grey geom while the materials are set, and no longer once they are cleared
    box = b.model.name2id('box', 'geom')
    px = on['rgb'][on['segmentation'][..., 0] == box]
    assert px.size and np.all(px[:, 0] > 100) and np.all(px[:, 1:] == 0)


def test_overrides_and_recolouring_reach_the_device(camera_lib):
  b = scene_batch(64)
  m = b.model
  cam = camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW, textures=True,
                               materials={'flat': dict(type='cube', builtin='checker', width=4, rgb1=(1, 1, 1), rgb2=(0, 0, 0)),
                                          'armg': dict(type='2d', builtin='checker', width=4, height=4)})
  assert cam.untextured == ['armg'] and cam.untextured_reasons == {'armg': '2d texture on a solid'}
  out = compare(b, cam, 'nearest', 'overrides')
  flat = m.name2id('flat', 'geom')
  px = out['rgb'][out['segmentation'][..., 0] == flat]
  assert px[:, 0].max() > 100 and px.max(axis=1).min() == 0      # red fields and black fields
  # a task recolours the model's texture on the host arrays: the next render draws it
  old = m.tex_rgb2[0].copy()
  try:
    m.tex_rgb2[0] = [0.1, 0.9, 0.1]
    after = images(cam)
  finally:
    m.tex_rgb2[0] = old
  floor = m.name2id('floor', 'geom')
  changed = np.any(after['rgb'] != out['rgb'], axis=-1)
  assert changed.any() and np.all(out['segmentation'][..., 0][changed] == floor)
  assert np.array_equal(images(cam)['rgb'], out['rgb'])
  with pytest.raises(ValueError, match='unknown material spec keys'):
    camera_lib.BatchCamera(b, ['down'], *HW, materials={'floor': dict(pattern='checker')})
  with pytest.raises(ValueError, match='texture_filter'):
    camera_lib.BatchCamera(b, ['down'], *HW, textures=True, texture_filter='bilinear')


def test_soccer_ball_and_skybox_textures(camera_lib):
  from dm_control_amd.batch import BatchedPhysics
  b = BatchedPhysics(mc.compile_xml(cs.soccer_xml()), B, precision=64, nconmax=24)
  rng = np.random.RandomState(5)
  b.set('ctrl', rng.uniform(-1, 1, (B, b.model.nu)))
  b.step(25)
  b.sync()
  names = ['home0/egocentric', 'soccer_ball/ball_cam_far', dict(body='home1/ball', pos=(1.5, 1.0, 0.6), mode='targetbody', target='home1/ball', fovy=45)]
  cam = camera_lib.BatchCamera(b, names, *cs.SOCCER_HW, textures=True)
  assert {'ground', 'soccer_ball/geom', 'home0/head', 'home1/head', 'away0/head', 'away1/head'} <= set(cam.untextured)
  assert set(cam.untextured_reasons.values()) == {'file texture'}
  out = compare(b, cam, 'nearest', 'soccer')
  plain = images(camera_lib.BatchCamera(b, names, *cs.SOCCER_HW))
  assert np.array_equal(plain['depth'], out['depth']) and np.array_equal(plain['segmentation'], out['segmentation'])
  seg = out['segmentation'][..., 0]
  shell = b.model.name2id('home1/shell', 'geom')
  assert (seg == shell).sum() > 50      # the close-up camera sees the player's ball body: two colours of fields on it
  assert len(np.unique(plain['rgb'][seg == shell] // 64, axis=0)) < len(np.unique(out['rgb'][seg == shell] // 64, axis=0))
  assert (seg < 0).any() and len(np.unique(out['rgb'][seg < 0], axis=0)) > 3 and len(np.unique(plain['rgb'][seg < 0], axis=0)) == 1


def test_pixel_environment_floor_moves_under_the_camera(camera_lib):
  import torch
  from dm_control_amd.suite import fused_env, pixels
  spec = dict(body='torso', pos=(0, -3, 0.5), xyaxes=(1, 0, 0, 0, 0, 1), mode='trackcom', fovy=45)

  env = fused_env.make('cheetah', 'run', 8)
  penv = pixels.wrap(env, [spec], 84, 84, materials={'ground': camera_lib.SUITE_GRID}, skybox=camera_lib.SUITE_SKYBOX, texture_filter='box')
  plain_cam = camera_lib.BatchCamera(penv.camera.batch, [spec], 84, 84)      # the same run without materials
  obs = penv.reset()
  act = torch.ones((8, env.model.nu), dtype=env.dtype, device=env.device)      # a constant forward action
  frames = []
  for k in range(2):      # the frame of the start state and the frame 20 control steps later
    for _ in range(20*k):
      obs = penv.step(act)[0]
    frames.append((obs.cpu().numpy(), penv.camera.render(segmentation=True)[..., 0].cpu().numpy(), penv.camera.batch.get('qpos')[:, 0].copy(),
                   plain_cam.render().cpu().numpy()))
  fa, fb = frames
  assert fa[0].shape == (8, 1, 84, 84, 3) and np.abs(fb[2] - fa[2]).min() > 1e-2      # every cheetah moved
  ground = penv.camera.model.name2id('ground', 'geom')

  def floor_region(sa, sb):
    """Ground in both frames, and so are the eight neighbours: away from the body's silhouette."""
    g = (sa == ground) & (sb == ground)
    inner = g.copy()
    for dr in (-1, 0, 1):
      for dc in (-1, 0, 1):
        inner &= np.roll(np.roll(g, dr, axis=-2), dc, axis=-1)
    inner[..., 0, :] = inner[..., -1, :] = False
    inner[..., :, 0] = inner[..., :, -1] = False
    return inner

  region = floor_region(fa[1], fb[1])
  assert region.reshape(8, -1).sum(1).min() > 200
  for e in range(8):
    assert np.any(fa[0][e][region[e]] != fb[0][e][region[e]]), e      # the patterned floor moved under the camera
  # the twin draws the same frame (box filter: the geom-edge rule alone)
  b = penv.camera.batch
  torch.cuda.synchronize()
  d, g, rgb, key, ex = ts.twin_images(b.model, penv.camera.cameras, 84, 84, read_state(b), 5, penv.camera.materials, penv.camera.sky, 'box')[0]
  assert ex.mean() <= EDGE_CAP
  assert np.abs(fb[0][5, 0][~ex].astype(int) - rgb[~ex].astype(int)).max() <= 1
  # the same run without materials: the floor region never changes
  assert np.array_equal(fa[3][region], fb[3][region]) and not np.array_equal(fa[3], fb[3])


def test_graph_replay_is_the_eager_render(camera_lib):
  import torch
  b = scene_batch(32)
  cam = camera_lib.BatchCamera(b, list(ts.CAMERAS), *HW, textures=True, texture_filter='box')
  eager = cam.render().clone()      # (the materials and colours are uploaded: nothing changes inside the capture)
  buf = torch.zeros_like(eager)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    cam.render(out=buf)
  buf.zero_()
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(buf, eager) and int(eager.max()) > 0

"""Ray-cast cameras, CPU tier: the numpy twin (tests/camera_twin.py) against the unchanged fp64 oracle's rangefinder
rays, the camera poses of every mode, the compiler's camera arrays, the edge rule's cap on the scenes the GPU tier uses,
and the host build of the kernel's per-pixel functions against the twin."""
import math

import numpy as np
import pytest

import camera_scenes as cs
import camera_twin as twin
from dm_control_amd import camera as camera_lib
from dm_control_amd import mjcf_compiler as mc
from oracle.oracle import OraclePhysics

TOL_F64 = 1e-9      # the project's fp64 tolerance (tests/test_gpu_parity.py TOL_F64_1000): both sides evaluate the same closed forms
EDGE_CAP = 0.03     # the edge rule may exclude at most this fraction of an image
STATE = ('geom_xpos', 'geom_xmat', 'xpos', 'xmat', 'subtree_com')
SIX_HW, SOCCER_HW = cs.SIX_HW, cs.SOCCER_HW


def oracle_state(p):
  return {k: np.array(getattr(p, k), dtype=np.float64)[None] for k in STATE}


def set_state(m, p, k):
  """State k of the six-primitive scene: the ball displaced and the arm swung; k = 2 hangs the ball on the optical axis
  of the `eye` camera, 0.6 m in front of it."""
  p.qpos[:3] += [0.1*k, -0.15*k, 0.2*k]
  p.qpos[7] = 0.6*k
  if k == 2:
    rig = m.name2id('rig', 'body')
    Rr = twin.quat_to_mat(m.body_quat[rig])
    p.qpos[:3] = m.body_pos[rig] + Rr @ np.array(cs.EYE_POS) + 0.6*(Rr @ twin.quat_to_mat(cs.EYE_QUAT) @ [0, 0, -1.0])
  p.forward()


def six_states():
  """Distinct states of the six-primitive scene: the ball displaced and turned, the arm swung."""
  m = mc.compile_xml(cs.six_primitive_xml())
  out = []
  for k in range(3):
    p = OraclePhysics(m)
    set_state(m, p, k)
    out.append(oracle_state(p))
  return m, out


def test_twin_depth_equals_the_oracles_rangefinder_rays():
  H, W = 6, 8
  R = twin.quat_to_mat(cs.EYE_QUAT)
  d = twin.pixel_dirs(cs.EYE_FOVY, H, W).reshape(-1, 3)
  sites = ''.join('<site name="px%d" pos="%s" zaxis="%s"/>' % (i, ' '.join(map(repr, cs.EYE_POS)), ' '.join(repr(float(v)) for v in R @ d[i]))
                  for i in range(H*W))
  sensors = '<sensor>%s</sensor>' % ''.join('<rangefinder site="px%d"/>' % i for i in range(H*W))
  m = mc.compile_xml(cs.six_primitive_xml((sites, sensors)))
  assert m.body_geomnum[m.name2id('rig', 'body')] == 0      # (a rangefinder skips its own body's geoms; the camera does not)
  seen = set()
  for k in range(3):
    p = OraclePhysics(m)
    set_state(m, p, k)
    cam = cs.resolve(m, ['eye'])
    depth, gid, _, _ = cs.twin_images(m, cam, H, W, oracle_state(p), 0)[0]
    sd = np.array(p.sensordata).reshape(H, W)
    cosang = (1 / np.linalg.norm(d, axis=1)).reshape(H, W)
    assert np.array_equal(sd < 0, gid < 0)      # misses are the sensor's -1
    assert np.all(sd[gid < 0] == -1) and np.all(np.isinf(depth[gid < 0]))
    hit = gid >= 0
    np.testing.assert_allclose(depth[hit], (sd*cosang)[hit], rtol=TOL_F64, atol=TOL_F64)
    seen |= set(int(m.geom_type[g]) for g in gid[hit])
    assert m.name2id('ghost', 'geom') not in gid      # alpha 0
  assert seen == set(twin.DRAWN), seen      # every primitive type was hit somewhere


def test_twin_fixed_pose_equals_the_facades_cam_xpos(monkeypatch):
  import oracle_backend as ob
  from dm_control_amd import mujoco_api as mj
  monkeypatch.setattr(mj, 'BatchedPhysics', ob.OracleBatch)      # (the facade's derived arrays on the CPU oracle)
  model = mj.MjModel.from_xml_string(cs.six_primitive_xml())
  data = mj.MjData(model)
  data.qpos[7] = 0.4
  mj.mj_forward(model, data)
  c = model._c
  i = c.name2id('eye', 'camera')
  cam = camera_lib.resolve_camera(c, 'eye')
  nb = c.nbody
  p, R = twin.camera_pose(cam['mode'], cam['body'], cam['target'], cam['pos'], cam['quat'], cam['pos0'], cam['poscom0'], cam['mat0'],
                          np.array(data.xpos).reshape(nb, 3), np.array(data.xmat).reshape(nb, 3, 3), np.array(data.subtree_com).reshape(nb, 3))
  np.testing.assert_allclose(p, np.array(data.cam_xpos)[i], atol=1e-12)
  np.testing.assert_allclose(R.ravel(), np.array(data.cam_xmat)[i].ravel(), atol=1e-12)
  # the shared derivation of the *0 constants is what the facade reports
  np.testing.assert_array_equal(np.array(model.cam_pos0), c.cam_pos0)
  np.testing.assert_array_equal(np.array(model.cam_poscom0), c.cam_poscom0)
  np.testing.assert_array_equal(np.array(model.cam_mat0), c.cam_mat0)


def _poses(m, st, names):
  cams = cs.resolve(m, names)
  nb = m.nbody
  args = (st['xpos'][0].reshape(nb, 3), st['xmat'][0].reshape(nb, 3, 3), st['subtree_com'][0].reshape(nb, 3))
  tw = [twin.camera_pose(c['mode'], c['body'], c['target'], c['pos'], c['quat'], c['pos0'], c['poscom0'], c['mat0'], *args) for c in cams]
  lib_p, lib_R = camera_lib.camera_poses(cams, st['xpos'], st['xmat'], st['subtree_com'])
  for k, (p, R) in enumerate(tw):      # the package's host poses (BatchCamera.matrices) agree with the twin
    np.testing.assert_allclose(lib_p[0, k], p, atol=1e-12)
    np.testing.assert_allclose(lib_R[0, k], R, atol=1e-12)
  return cams, tw


def test_twin_tracking_poses_keep_mat0_and_follow_the_body():
  m, states = six_states()
  ball, arm = m.name2id('ball', 'body'), m.name2id('arm', 'body')
  ref = None
  for st in states:
    cams, ((pt, Rt), (pc, Rc)) = _poses(m, st, ['track', 'trackcom'])
    np.testing.assert_allclose(Rt.ravel(), cams[0]['mat0'], atol=1e-14)
    np.testing.assert_allclose(Rc.ravel(), cams[1]['mat0'], atol=1e-14)
    off = (pt - st['xpos'][0].reshape(-1, 3)[ball], pc - st['subtree_com'][0].reshape(-1, 3)[arm])
    if ref is None:
      ref = off
      # at qpos0 the tracking pose is the fixed pose
      fixed = [dict(c, mode=0) for c in cams]
      pf, Rf = camera_lib.camera_poses(fixed, st['xpos'], st['xmat'], st['subtree_com'])
      np.testing.assert_allclose(pf[0, 0], pt, atol=1e-12)
      np.testing.assert_allclose(Rf[0, 0], Rt, atol=1e-12)
      np.testing.assert_allclose(pf[0, 1], pc, atol=1e-12)
    np.testing.assert_allclose(off[0], ref[0], atol=1e-12)
    np.testing.assert_allclose(off[1], ref[1], atol=1e-12)
  assert np.abs(states[2]['subtree_com'][0].reshape(-1, 3)[arm] - states[0]['subtree_com'][0].reshape(-1, 3)[arm]).max() > 0.05


def test_targetbody_projects_its_target_onto_the_image_centre():
  m, states = six_states()
  H, W = 48, 64
  ball, arm = m.name2id('ball', 'body'), m.name2id('arm', 'body')
  for st in states:
    cams, tw = _poses(m, st, ['target', 'targetcom'])
    pos, mat = camera_lib.camera_poses(cams, st['xpos'], st['xmat'], st['subtree_com'])
    M = camera_lib.camera_matrices(cams, pos, mat, H, W)
    for k, tgt in enumerate((st['xpos'][0].reshape(-1, 3)[ball], st['subtree_com'][0].reshape(-1, 3)[arm])):
      x, y, w = M[0, k] @ np.append(tgt, 1.0)
      np.testing.assert_allclose([x/w, y/w], [(W - 1)/2, (H - 1)/2], atol=1e-9)
      assert w < 0      # in front of the camera: w is the camera-frame z, and the camera looks down -z
      R = tw[k][1]
      np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-12)
      assert abs(R[2, 0]) < 1e-12 and np.linalg.det(R) > 0      # x axis horizontal, right-handed


def test_camera_matrix_agrees_with_the_pixel_rays():
  # a world point on the ray of pixel (r, c) projects back to (c, r): matrices() and the render share one pinhole model
  m, states = six_states()
  st = states[1]
  H, W = 6, 8
  cams = cs.resolve(m, ['eye'])
  pos, mat = camera_lib.camera_poses(cams, st['xpos'], st['xmat'], st['subtree_com'])
  M = camera_lib.camera_matrices(cams, pos, mat, H, W)[0, 0]
  d = twin.pixel_dirs(cs.EYE_FOVY, H, W)
  for r, c in ((0, 0), (5, 7), (2, 3)):
    x, y, w = M @ np.append(pos[0, 0] + 2.5*(mat[0, 0] @ d[r, c]), 1.0)
    np.testing.assert_allclose([x/w, y/w], [c, r], atol=1e-9)


def test_compiler_camera_arrays_small_model():
  m = mc.compile_xml(cs.six_primitive_xml())
  assert [m.names['camera'][i] for i in range(m.ncam)] == ['track', 'trackcom', 'eye', 'target', 'targetcom']
  assert list(m.cam_mode) == [1, 2, 0, 3, 4]
  assert list(m.cam_targetbodyid) == [-1, -1, -1, m.name2id('ball', 'body'), m.name2id('arm', 'body')]
  assert m.geom_group[m.name2id('hidden', 'geom')] == 3 and m.geom_group.sum() == 3
  assert m.geom_matid[m.name2id('painted', 'geom')] == 0 and (m.geom_matid >= 0).sum() == 1
  assert m.cam_pos0.shape == (5, 3) and m.cam_poscom0.shape == (5, 3) and m.cam_mat0.shape == (5, 9)
  # a camera on a static body: offset from the body origin = the body's rotation applied to cam_pos
  rig = m.name2id('rig', 'body')
  np.testing.assert_allclose(m.cam_pos0[2], mc.rot_vec(m.body_quat[rig], m.cam_pos[2]), atol=1e-14)
  np.testing.assert_allclose(m.cam_mat0[2], mc.quat_to_mat(mc.quat_mul(m.body_quat[rig], m.cam_quat[2])).ravel(), atol=1e-14)
  # the ball is one sphere: its subtree COM is its origin
  np.testing.assert_allclose(m.cam_poscom0[0], m.cam_pos0[0], atol=1e-14)
  with pytest.raises(mc.MjcfError, match='target'):
    mc.compile_xml('<mujoco><worldbody><camera mode="targetbody"/></worldbody></mujoco>')


def test_compiler_camera_arrays_soccer():
  m = mc.compile_xml(cs.soccer_xml())
  assert m.ncam == 16
  names = m.names['camera']
  modes = dict(zip(names, m.cam_mode))
  assert modes['top_down'] == 0 and modes['soccer_ball/ball_cam'] == 2 and modes['home0/egocentric'] == 0
  assert modes['home0/tracking'] == 2 and modes['away1/float_far'] == 0
  assert sorted(m.cam_mode) == [0]*9 + [2]*7
  assert np.all(m.cam_targetbodyid == -1)
  assert m.geom_group.shape == (m.ngeom,) and set(m.geom_group) == {0, 5}
  assert m.cam_pos0.shape == (16, 3) and m.cam_mat0.shape == (16, 9)
  # top_down hangs 95 m above the world origin and looks down its -z
  i = names.index('top_down')
  np.testing.assert_allclose(m.cam_pos0[i], [0, 0, 95], atol=1e-12)
  np.testing.assert_allclose(m.cam_mat0[i].reshape(3, 3)[:, 2], [0, 0, 1], atol=1e-12)


def test_user_camera_specs():
  m = mc.compile_xml(cs.six_primitive_xml())
  c = camera_lib.resolve_camera(m, dict(body='ball', pos=(0, -1, 0), zaxis=(0, -1, 0), mode='trackcom', fovy=30))
  assert c['mode'] == 2 and c['body'] == m.name2id('ball', 'body')
  np.testing.assert_allclose(twin.quat_to_mat(c['quat'])[:, 2], [0, -1, 0], atol=1e-12)
  c = camera_lib.resolve_camera(m, dict(xyaxes=(0, 1, 0, 0, 0, 2)))
  np.testing.assert_allclose(twin.quat_to_mat(c['quat']), [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-12)
  assert camera_lib.resolve_camera(m, 2)['name'] == 'eye'
  for bad in (dict(mode='targetbody'), dict(quat=(1, 0, 0, 0), zaxis=(0, 0, 1)), dict(fovy=0), dict(colour=1)):
    with pytest.raises(ValueError):
      camera_lib.resolve_camera(m, bad)
  with pytest.raises(ValueError):
    camera_lib.resolve_camera(m, 'nope')


def test_edge_rule_excludes_at_most_three_percent_six_primitives():
  m, states = six_states()
  cams = cs.resolve(m, cs.SIX_CAMERAS)
  for st in states:
    for name, (_, gid, _, ex) in zip(cs.SIX_CAMERAS, cs.twin_images(m, cams, *SIX_HW, st, 0)):
      assert ex.mean() <= EDGE_CAP, (name, ex.mean())
      assert (gid >= 0).mean() > 0.02, name      # (the camera looks at the scene)


def test_edge_rule_excludes_at_most_three_percent_soccer():
  m = mc.compile_xml(cs.soccer_xml())
  p = OraclePhysics(m)
  p.forward()
  cams = cs.resolve(m, cs.SOCCER_CAMERAS)
  for c, (_, gid, _, ex) in zip(cs.SOCCER_CAMERAS, cs.twin_images(m, cams, *SOCCER_HW, oracle_state(p), 0)):
    assert ex.mean() <= EDGE_CAP, (c, ex.mean())
    assert (gid >= 0).mean() > 0.2, c


CHEETAH_CAMERA = dict(body='torso', pos=(0, -3, 0.5), xyaxes=(1, 0, 0, 0, 0, 1), mode='trackcom', fovy=45)


def test_edge_rule_excludes_at_most_three_percent_cheetah():
  # the scene of the pixels.wrap test of the GPU tier: cheetah, one user trackcom camera, 84 x 84
  import os
  with open(os.path.join(cs.ROOT, 'dm_control_amd', 'suite', 'assets', 'cheetah.xml')) as f:
    m = mc.compile_xml(f.read())
  rs = np.random.RandomState(1)
  for k in range(3):
    p = OraclePhysics(m)
    p.qpos[3:] += rs.uniform(-0.4, 0.4, m.nq - 3)
    p.qpos[0] += k
    p.forward()
    _, gid, _, ex = cs.twin_images(m, cs.resolve(m, [CHEETAH_CAMERA]), 84, 84, oracle_state(p), 0)[0]
    assert ex.mean() <= EDGE_CAP, ex.mean()
    assert (gid >= 0).mean() > 0.05


@pytest.mark.parametrize('prec', [64, 32])
def test_host_build_of_the_device_functions_matches_the_twin(prec):
  import camera_emu_lib as emu
  m, states = six_states()
  cams = cs.resolve(m, cs.SIX_CAMERAS)
  H, W = SIX_HW
  worst = 0.0
  for st in states:
    tw = cs.twin_images(m, cams, H, W, st, 0)
    em = cs.twin_images(m, cams, H, W, st, 0, fn=lambda *a, **k: emu.render(prec, *a, **k))
    for c, (d, g, rgb, ex), (de, ge, rgbe) in zip(cams, tw, em):
      keep = ~ex
      assert np.array_equal(g[keep], ge[keep]), c['name']
      hit = keep & (g >= 0)
      err = np.abs(de[hit] - d[hit]) / np.maximum(1, d[hit])
      worst = max(worst, err.max())
      assert np.all(np.isinf(de[keep & (g < 0)]))
      assert np.abs(rgbe[keep].astype(int) - rgb[keep].astype(int)).max() <= 1, c['name']
      # the device pose function against the twin's
      nb = m.nbody
      p, R = emu.pose(c, st['xpos'][0], st['xmat'][0], st['subtree_com'][0])
      pt, Rt = twin.camera_pose(c['mode'], c['body'], c['target'], c['pos'], c['quat'], c['pos0'], c['poscom0'], c['mat0'],
                                st['xpos'][0].reshape(nb, 3), st['xmat'][0].reshape(nb, 3, 3), st['subtree_com'][0].reshape(nb, 3))
      np.testing.assert_allclose(p, pt, atol=1e-12)
      np.testing.assert_allclose(R, Rt, atol=1e-12)
  print('host build, fp%d: max |d depth| / max(1, depth) = %.3g' % (prec, worst))
  # fp64: the project's fp64 tolerance; fp32: the bound of the GPU tier, 4 x the 1.303e-6 measured on the device for this scene
  # (this host build measures 1.1e-6)
  assert worst < (TOL_F64 if prec == 64 else 4 * 1.303e-6), worst


def test_near_far_and_groups_in_the_twin_and_host_build():
  import camera_emu_lib as emu
  m, states = six_states()
  cams = cs.resolve(m, ['eye'])
  H, W = SIX_HW
  base = cs.twin_images(m, cams, H, W, states[0], 0)[0]
  clip = cs.twin_images(m, cams, H, W, states[0], 0, near=1.9, far=2.6)[0]
  assert np.all((clip[0][clip[1] >= 0] >= 1.9) & (clip[0][clip[1] >= 0] <= 2.6))
  assert np.all(clip[0][clip[1] < 0] == 2.6) and (base[0] < 1.9).any()
  e = cs.twin_images(m, cams, H, W, states[0], 0, near=1.9, far=2.6, fn=lambda *a, **k: emu.render(64, *a, **k))[0]
  keep = ~(base[3] | clip[3])
  assert np.array_equal(e[1][keep], clip[1][keep])
  allg = cs.twin_images(m, cams, H, W, states[0], 0, visible=cs.visible_mask(m, (0, 1, 2, 3)))[0]
  hidden = m.name2id('hidden', 'geom')
  assert hidden in allg[1] and hidden not in base[1]

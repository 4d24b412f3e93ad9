"""TEST INFRASTRUCTURE: the scenes of the camera tests (CPU and GPU tiers) and the glue between a state -- the oracle's or
a device batch's -- and the numpy twin."""
import os

import numpy as np

import camera_twin as twin
from dm_control_amd import camera as camera_lib
from dm_control_amd import mjcf_compiler as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the rotated camera on the geom-less static body `rig` (the oracle comparison puts one rangefinder site per pixel there)
EYE_POS = (0.05, -0.02, 0.1)
EYE_QUAT = (0.8804762, 0.4402381, -0.1320714, -0.1188643)
EYE_FOVY = 50.0


def six_primitive_xml(sites=''):
  """Every primitive type, a finite plane, an alpha-0 geom in front of the camera, a hidden-group geom, a geom coloured
  by its material, a free ball and a hinged arm; cameras of all five modes."""
  return """<mujoco><option timestep="0.005"/>
  <asset><material name="red" rgba=".8 .1 .1 1"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="1.6 1.4 .1" rgba=".3 .5 .3 1"/>
    <geom name="cyl" type="cylinder" size=".15 .2" pos=".55 .1 .2" quat=".98 .1 .15 0" rgba=".2 .3 .9 1"/>
    <geom name="box" type="box" size=".15 .1 .2" pos="-.35 .45 .2" quat=".9 0 0 .43" rgba=".9 .8 .2 1"/>
    <geom name="ghost" type="sphere" size=".3" pos="-.9 -.9 1.1" rgba="1 0 0 0"/>
    <geom name="ell" type="ellipsoid" size=".1 .2 .3" pos="-.5 -.3 .3" quat=".95 .2 0 .2" rgba=".7 .2 .7 1"/>
    <geom name="cap" type="capsule" size=".07 .2" pos=".2 -.45 .3" quat=".8 .5 .3 0" rgba=".1 .8 .8 1"/>
    <geom name="hidden" type="sphere" size=".12" pos="0 0 .12" group="3" rgba="1 1 1 1"/>
    <geom name="painted" type="sphere" size=".1" pos=".1 .5 .1" material="red"/>
    <body name="ball" pos=".15 .05 .6"><freejoint name="ballj"/><geom name="ballg" type="sphere" size=".1" rgba=".9 .4 .1 1"/>
      <camera name="track" mode="track" pos="-.8 -.9 .7" xyaxes="1 -.9 0 .4 .5 1" fovy="55"/></body>
    <body name="arm" pos=".6 .6 .7"><joint name="hinge" type="hinge" axis="0 1 0"/>
      <geom name="armg" type="capsule" fromto="0 0 0 -.35 0 -.1" size=".04" rgba=".6 .6 .6 1"/>
      <camera name="trackcom" mode="trackcom" pos=".9 .8 .6" xyaxes="-.8 1 0 -.4 -.4 1" fovy="60"/></body>
    <body name="rig" pos="-1.3 -1.1 1.3" quat=".9 .1 .2 -.35">
      <camera name="eye" pos="%s" quat="%s" fovy="%g"/>
      <camera name="target" mode="targetbody" target="ball" pos="2.3 .3 .2" fovy="40"/>
      <camera name="targetcom" mode="targetbodycom" target="arm" pos=".3 2.0 .1" fovy="45"/>%s</body>
  </worldbody>%s</mujoco>""" % (' '.join(map(str, EYE_POS)), ' '.join(map(str, EYE_QUAT)), EYE_FOVY, sites[0] if sites else '',
                                sites[1] if sites else '')


SIX_CAMERAS = ('eye', 'track', 'trackcom', 'target', 'targetcom')
SIX_HW = (48, 64)


def soccer_xml():
  with open(os.path.join(ROOT, 'dm_control_amd', 'suite', 'assets', 'soccer_2v2_boxhead.xml')) as f:
    return f.read()


# fixed, egocentric and trackcom cameras of the file, plus user cameras for the modes the file does not use
SOCCER_CAMERAS = ('home0/egocentric', 'away1/egocentric', 'soccer_ball/ball_cam_far', 'home1/float_far',
                  dict(body=0, pos=(12, -10, 8), mode='targetbody', target='soccer_ball/', fovy=30),
                  dict(body=0, pos=(-10, 12, 6), mode='targetbodycom', target='home0/', fovy=30),
                  dict(body='soccer_ball/', pos=(6, 4, 4), xyaxes=(-1, 1.5, 0, -.5, -.3, 1), mode='track', fovy=60))
# tall images: a level egocentric camera over the pitch has a horizon, and the rows within two pixels of it fall under the
# edge rule whatever the resolution (depth = height / tan(angle below the horizon))
SOCCER_HW = (120, 64)
SOCCER_EGOCENTRIC = ('home0/egocentric', 'home1/egocentric', 'away0/egocentric', 'away1/egocentric')


def visible_mask(model, geom_groups=(0, 1, 2)):
  return np.array([int(model.geom_type[g]) in twin.DRAWN and not model.geom_invisible[g] and int(model.geom_group[g]) in geom_groups
                   for g in range(model.ngeom)], dtype=bool)


def twin_images(model, cams, H, W, state, env, geom_size=None, fn=twin.render, **kw):
  """The twin's (depth, gid, rgb, excluded) per camera for environment `env` of `state` = dict of (B, rows) arrays geom_xpos,
  geom_xmat, xpos, xmat, subtree_com.  cams: resolved cameras (camera.resolve_camera)."""
  nb, ng = model.nbody, model.ngeom
  xpos = state['xpos'][env].reshape(nb, 3)
  xmat = state['xmat'][env].reshape(nb, 3, 3)
  com = state['subtree_com'][env].reshape(nb, 3)
  gpos = state['geom_xpos'][env].reshape(ng, 3)
  gmat = state['geom_xmat'][env].reshape(ng, 3, 3)
  size = np.asarray(model.geom_size if geom_size is None else geom_size, dtype=np.float64).reshape(ng, 3)
  vis = kw.pop('visible', None)
  vis = visible_mask(model) if vis is None else vis
  color = kw.pop('color', None)
  if color is None:
    color = twin.effective_colors(model.geom_rgba, model.geom_matid, model.mat_rgba)
  out = []
  for c in cams:
    p, R = twin.camera_pose(c['mode'], c['body'], c['target'], c['pos'], c['quat'], c['pos0'], c['poscom0'], c['mat0'], xpos, xmat, com)
    if fn is not twin.render:
      out.append(fn(p, R, c['fovy'], H, W, model.geom_type, size, gpos, gmat, vis, color, **kw))
      continue
    f = lambda dx, dy, p=p, R=R, c=c: twin.render(p, R, c['fovy'], H, W, model.geom_type, size, gpos, gmat, vis, color, dx=dx, dy=dy, **kw)
    out.append(f(0.0, 0.0) + (twin.excluded(f),))
  return out


def resolve(model, cams):
  return [camera_lib.resolve_camera(model, c) for c in cams]

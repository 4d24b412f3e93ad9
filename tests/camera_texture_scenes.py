"""TEST INFRASTRUCTURE: the textured scene of the camera texture tests (CPU and GPU tiers) and the glue between a state
and the texture twin.  Coarse textures (8 x 8, 4 x 4, 5 x 5 texels) on geoms near the cameras, so that at 20 x 28 pixels
the edge rule with its texel-class extension stays under its 3 % cap."""
import numpy as np

import camera_scenes as cs
import camera_texture_twin as ttwin
import camera_twin as twin
from dm_control_amd import camera as camera_lib

HW = (20, 28)      # 560 pixels: three tiles of the render kernel, the last one partial, rows split across tile boundaries
CAMERAS = ('down', 'follow')
PLANE_CASES = (('false', '1 1'), ('true', '.6 .45'))      # (texuniform, texrepeat) of the floor's material


def textured_xml(texuniform='false', texrepeat='1 1'):
  """A finite plane with a 2d checker and edge marks; a box with a cube texture of cross marks, a capsule with a
  cube checker, a free sphere with a 2 x 2 cube checker tinted by its material's rgba; a flat-coloured cylinder; a gradient skybox; a fixed camera looking
  down at an angle and a trackcom camera on the ball."""
  return """<mujoco><option timestep="0.005"/>
  <asset>
    <texture name="tiles" type="2d" builtin="checker" rgb1=".9 .9 .9" rgb2=".2 .3 .8" mark="edge" markrgb=".9 .1 .1" width="8" height="8"/>
    <texture name="cubes" type="cube" builtin="checker" rgb1=".9 .7 .1" rgb2=".1 .1 .1" width="4" height="4"/>
    <texture name="crossed" type="cube" builtin="flat" rgb1="1 1 1" mark="cross" markrgb="0 0 .6" width="5" height="5"/>
    <texture name="sky" type="skybox" builtin="gradient" rgb1=".4 .6 .8" rgb2=".05 .05 .1" width="64" height="64"/>
    <material name="tiles" texture="tiles" texrepeat="%s" texuniform="%s"/>
    <material name="cubes" texture="cubes"/>
    <texture name="halves" type="cube" builtin="checker" rgb1=".2 .8 .3" rgb2=".95 .95 .95" width="2" height="2"/>
    <material name="crossed" texture="crossed"/>
    <material name="halves" texture="halves" rgba=".9 1 .8 1"/>
    <material name="plain" rgba=".8 .2 .2 1"/>
  </asset>
  <worldbody>
    <geom name="floor" type="plane" size="1.2 1 .1" material="tiles"/>
    <geom name="box" type="box" size=".2 .15 .25" pos="-.5 .3 .25" quat=".9 0 0 .43" material="crossed"/>
    <geom name="flat" type="cylinder" size=".12 .2" pos=".6 .45 .2" material="plain"/>
    <body name="ball" pos=".1 -.1 .5"><freejoint name="ballj"/><geom name="ballg" type="sphere" size=".18" material="halves"/>
      <camera name="follow" mode="trackcom" pos="-.75 -.6 .6" xyaxes="1 -1.2 0 .5 .4 1" fovy="55"/></body>
    <body name="arm" pos=".55 -.4 .6"><joint name="hinge" type="hinge" axis="0 1 0"/>
      <geom name="armg" type="capsule" fromto="0 0 0 -.3 0 -.1" size=".08" material="cubes"/></body>
    <camera name="down" pos=".5 -2 2" xyaxes="2 .5 0 -.9 3.6 4.25" fovy="32"/>
  </worldbody></mujoco>""" % (texrepeat, texuniform)


def env_qpos(model, B):
  """A different state per environment: the ball displaced and turned, the arm swung."""
  q = np.tile(model.qpos0, (B, 1))
  k = np.arange(B)
  q[:, 0] += 0.12*k - 0.1
  q[:, 1] -= 0.08*k
  q[:, 2] += 0.05*k
  q[:, 3:7] = np.array([[1, 0, 0, 0], [.9, .3, .2, .1], [.7, -.2, .5, .3]])[k % 3]
  q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
  q[:, 7] = 0.5*k - 0.4
  return q


NSTEP = 6      # steps the GPU tier takes from env_qpos before it renders
STATE = ('geom_xpos', 'geom_xmat', 'xpos', 'xmat', 'subtree_com')


def oracle_states(model, B, nstep=NSTEP):
  """The state dicts (one environment each) the CPU tier renders: env_qpos stepped on the fp64 oracle."""
  from oracle.oracle import OraclePhysics
  out = []
  for q in env_qpos(model, B):
    p = OraclePhysics(model)
    p.qpos[:] = q
    p.forward()
    p.step(nstep)
    p.forward()
    out.append({k: np.array(getattr(p, k), dtype=np.float64)[None] for k in STATE})
  return out


def twin_images(model, cams, H, W, state, env, specs, sky, texture_filter='nearest', fn=None, geom_groups=(0, 1, 2), **kw):
  """Per camera the texture twin's (depth, gid, rgb, key, excluded) for environment `env` of `state` (camera_scenes.twin_images'
  state dict); with fn (a host build's render) its (depth, gid, rgb).  Under 'box' only the geom-edge rule excludes."""
  nb, ng = model.nbody, model.ngeom
  xpos, xmat = state['xpos'][env].reshape(nb, 3), state['xmat'][env].reshape(nb, 3, 3)
  com = state['subtree_com'][env].reshape(nb, 3)
  gpos, gmat = state['geom_xpos'][env].reshape(ng, 3), state['geom_xmat'][env].reshape(ng, 3, 3)
  size = np.asarray(model.geom_size, dtype=np.float64).reshape(ng, 3)
  vis = cs.visible_mask(model, geom_groups)
  color = twin.effective_colors(model.geom_rgba, model.geom_matid, model.mat_rgba)
  out = []
  for c in cams:
    p, R = twin.camera_pose(c['mode'], c['body'], c['target'], c['pos'], c['quat'], c['pos0'], c['poscom0'], c['mat0'], xpos, xmat, com)
    if fn is not None:
      out.append(fn(p, R, c['fovy'], H, W, model.geom_type, size, gpos, gmat, vis, color, specs, sky, texture_filter, **kw))
      continue
    f = lambda dx, dy, p=p, R=R, c=c: ttwin.render(p, R, c['fovy'], H, W, model.geom_type, size, gpos, gmat, vis, color, specs, sky,
                                                   texture_filter, dx=dx, dy=dy, **kw)
    out.append(f(0.0, 0.0) + (ttwin.excluded(f),))
  return out


def model_materials(model, **kw):
  """(specs per geom, sky spec) as BatchCamera(textures=True, **kw) resolves them."""
  res = camera_lib.resolve_materials(model, True, kw.get('materials'), kw.get('skybox'))
  return res['geoms'], res['sky']

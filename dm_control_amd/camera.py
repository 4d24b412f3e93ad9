"""BatchCamera: ray-cast cameras for a whole batch, rendered on the device by one HIP launch.

The reference renders one environment at a time through OpenGL (`engine.Camera`, dm_control/mujoco/engine.py:700-946;
`suite/wrappers/pixels.py`).  This module gives a batch what pixel-based agents need from that -- depth, segmentation
and RGB images of every environment, as torch tensors that never leave the GPU -- with a GEOMETRIC camera:

  * pinhole model of engine.py:790-795: f = 0.5 H / tan(fovy / 2); pixel (row r, col c), row 0 at the top, looks along
    the camera-frame direction ((c - (W - 1) / 2) / f, -(r - (H - 1) / 2) / f, -1);
  * depth: the ray parameter of the nearest hit with that unnormalised direction = metres along the optical axis (what
    engine.py:924 returns); `far` where nothing is hit; hits nearer than `near` or beyond `far` are skipped;
  * segmentation: (geom id, 5 = mjOBJ_GEOM), background (-1, -1);
  * RGB: NOT OpenGL.  The geom's colour (geom_rgba, or its material's rgba where the geom's own is MuJoCo's default
    grey) under a headlight at the camera: colour * (ambient + diffuse * max(0, n . -d)), rounded as
    floor(255 clip(x, 0, 1) + 0.5), over a constant background.  No lights, shadows, reflections, sites or tendons.
  * textures (opt-in: `textures`, `materials`, `skybox`, `texture_filter`): the BUILTIN patterns of <texture> -- flat,
    checker, gradient, with edge / cross marks -- evaluated analytically per pixel on the final hit, texel x colour under
    the same headlight; 2d textures on planes (texrepeat / texuniform as in mjModel), cube textures on the solids (the
    face is the largest local coordinate), a flat / gradient skybox where nothing is hit; 'box' filtering takes the exact
    mean of the pattern over the pixel's footprint on a plane.  The model is PARITY_ASSUMPTIONS.md's, not OpenGL's.
    File textures are not decoded, `mark="random"` is ignored, and a texture on a geom type it does not map onto keeps
    the flat colour (`untextured`).  Depth and segmentation never depend on any of this.
  * drawn: plane (front side only, finite where its half-sizes are positive), sphere, capsule, ellipsoid, cylinder,
    box.  Mesh and height-field geoms are scenery the camera does not draw (`skipped_geoms`).  Geoms with alpha 0 and
    geoms whose group is not in `geom_groups` are invisible.  A camera sees the geoms of its own body.

Camera poses follow mjModel's five modes per environment (`camera_poses`), from the xpos / xmat / subtree_com the last
step or forward launch wrote; geom sizes are the ones the step kernel uses (after `set_model_real`, and per environment
for `set_env_geoms` geoms).
"""
import ctypes
import logging
import math

import numpy as np

from dm_control_amd import _native
from dm_control_amd import _unit
from dm_control_amd import mjcf_compiler

MODES = ('fixed', 'track', 'trackcom', 'targetbody', 'targetbodycom')
RGB, DEPTH, SEG = 1, 2, 4
_find_batch = _unit.find_batch      # (its earlier home)


class _Spec(ctypes.Structure):      # dmc_camera_spec
  _fields_ = [('mode', ctypes.c_int32), ('bodyid', ctypes.c_int32), ('targetbodyid', ctypes.c_int32), ('reserved', ctypes.c_int32),
              ('pos', ctypes.c_double * 3), ('mat', ctypes.c_double * 9), ('pos0', ctypes.c_double * 3),
              ('poscom0', ctypes.c_double * 3), ('mat0', ctypes.c_double * 9), ('fovy', ctypes.c_double)]


class _Material(ctypes.Structure):      # dmc_camera_material
  _fields_ = [('mapping', ctypes.c_int32), ('builtin', ctypes.c_int32), ('mark', ctypes.c_int32), ('width', ctypes.c_int32),
              ('height', ctypes.c_int32), ('texuniform', ctypes.c_int32), ('has_rgba', ctypes.c_int32), ('reserved', ctypes.c_int32),
              ('rgb1', ctypes.c_double * 3), ('rgb2', ctypes.c_double * 3), ('markrgb', ctypes.c_double * 3),
              ('texrepeat', ctypes.c_double * 2), ('rgba', ctypes.c_double * 4)]


class _Sky(ctypes.Structure):      # dmc_camera_sky
  _fields_ = [('builtin', ctypes.c_int32), ('reserved', ctypes.c_int32), ('rgb1', ctypes.c_double * 3), ('rgb2', ctypes.c_double * 3)]


class _Options(ctypes.Structure):      # dmc_camera_options
  _fields_ = [('near_m', ctypes.c_double), ('far_m', ctypes.c_double), ('ambient', ctypes.c_double), ('diffuse', ctypes.c_double),
              ('background', ctypes.c_double * 3), ('group_mask', ctypes.c_int32), ('nmat', ctypes.c_int32),
              ('geom_group', ctypes.c_void_p), ('geom_matid', ctypes.c_void_p)]


# The suite's floor and sky: the values of the reference's suite/common/materials.xml:8-9 (texture and material `grid`)
# and suite/common/skybox.xml:3-4, restated as material specs.
SUITE_GRID = dict(type='2d', builtin='checker', rgb1=(0.1, 0.2, 0.3), rgb2=(0.2, 0.3, 0.4), width=300, height=300, mark='edge',
                  markrgb=(0.2, 0.3, 0.4), texrepeat=(1.0, 1.0), texuniform=True)
SUITE_SKYBOX = dict(type='skybox', builtin='gradient', rgb1=(0.4, 0.6, 0.8), rgb2=(0.0, 0.0, 0.0), width=800, height=800,
                    mark='random', markrgb=(1.0, 1.0, 1.0))
FILTERS = ('nearest', 'box')
_SPEC_KEYS = frozenset(('builtin', 'type', 'rgb1', 'rgb2', 'mark', 'markrgb', 'width', 'height', 'texrepeat', 'texuniform', 'rgba'))
_SPEC_DEFAULTS = dict(type='cube', builtin='none', rgb1=(0.8, 0.8, 0.8), rgb2=(0.5, 0.5, 0.5), mark='none', markrgb=(0.0, 0.0, 0.0),
                      width=0, height=0, texrepeat=(1.0, 1.0), texuniform=False, rgba=None)
_DEV_BUILTIN = {'flat': 0, 'checker': 1, 'gradient': 2}      # CAM_TEX_*
_DEV_MARK = {'none': 0, 'random': 0, 'edge': 1, 'cross': 2}      # CAM_MARK_*
_TEX_ARRAYS = ('tex_type', 'tex_builtin', 'tex_rgb1', 'tex_rgb2', 'tex_mark', 'tex_markrgb', 'tex_width', 'tex_height', 'tex_file',
               'mat_texid', 'mat_texrepeat', 'mat_texuniform')


def material_spec(spec):
  """A complete material spec (every key of _SPEC_DEFAULTS) from a user's partial one; ValueError on unknown keys or
  values."""
  unknown = set(spec) - _SPEC_KEYS
  if unknown:
    raise ValueError('unknown material spec keys: %s' % sorted(unknown))
  out = dict(_SPEC_DEFAULTS, **spec)
  for key, allowed in (('type', mjcf_compiler.TEX_TYPES), ('builtin', mjcf_compiler.TEX_BUILTINS), ('mark', mjcf_compiler.TEX_MARKS)):
    if out[key] not in allowed:
      raise ValueError('material spec %s=%r: expected one of %s' % (key, out[key], list(allowed)))
  for key, n in (('rgb1', 3), ('rgb2', 3), ('markrgb', 3), ('texrepeat', 2)):
    out[key] = tuple(float(v) for v in np.asarray(out[key], dtype=np.float64).reshape(n))
  if out['rgba'] is not None:
    out['rgba'] = tuple(float(v) for v in np.asarray(out['rgba'], dtype=np.float64).reshape(4))
  out['width'], out['height'], out['texuniform'] = int(out['width']), int(out['height']), bool(out['texuniform'])
  return out


def _model_texture(model, t):
  """Texture t of the model as a spec without the material's keys, and whether its texels come from files."""
  return dict(type=mjcf_compiler.TEX_TYPES[int(model.tex_type[t])], builtin=mjcf_compiler.TEX_BUILTINS[int(model.tex_builtin[t])],
              rgb1=tuple(model.tex_rgb1[t]), rgb2=tuple(model.tex_rgb2[t]), mark=mjcf_compiler.TEX_MARKS[int(model.tex_mark[t])],
              markrgb=tuple(model.tex_markrgb[t]), width=int(model.tex_width[t]), height=int(model.tex_height[t])), bool(model.tex_file[t])


def resolve_materials(model, textures=True, materials=None, skybox=None):
  """What the cameras draw on every geom and in the sky.  textures: use the model's own <texture> / <material>
  declarations; materials: {geom name or id: spec} overriding or adding per geom; skybox: a spec.  Returns dict(
  geoms = per geom a complete spec or None (flat colour), sky = a complete spec or None (constant background),
  untextured = the geoms whose texture is not drawn, reasons = {geom: why}, ignored_marks = who asked for mark="random")."""
  names = model.names.get('geom', [None] * model.ngeom)
  label = lambda g: names[g] if names[g] is not None else g
  geoms, filed = [None] * model.ngeom, [False] * model.ngeom
  if textures:
    for g in range(model.ngeom):
      mat = int(model.geom_matid[g])
      t = int(model.mat_texid[mat]) if mat >= 0 else -1
      if t >= 0:
        tex, filed[g] = _model_texture(model, t)
        geoms[g] = material_spec(dict(tex, texrepeat=tuple(model.mat_texrepeat[mat]), texuniform=bool(model.mat_texuniform[mat])))
  for key, spec in (materials or {}).items():
    g = model.name2id(key, 'geom') if isinstance(key, str) else int(key)
    if not 0 <= g < model.ngeom:
      raise ValueError('materials: geom id %d out of range' % g)
    geoms[g], filed[g] = material_spec(spec), False
  sky = None
  if skybox is not None:
    sky = material_spec(dict(skybox))
    if sky['builtin'] not in ('gradient', 'flat'):
      raise ValueError('skybox: builtin must be gradient or flat')
  elif textures:
    for t in range(model.ntex):
      if mjcf_compiler.TEX_TYPES[int(model.tex_type[t])] == 'skybox':
        tex, from_file = _model_texture(model, t)
        if not from_file and tex['builtin'] in ('gradient', 'flat'):
          sky = material_spec(tex)
        break
  untextured, reasons, ignored = [], {}, []
  for g, spec in enumerate(geoms):
    if spec is None:
      continue
    gtype = int(model.geom_type[g])
    why = None
    if filed[g]:
      why = 'file texture'
    elif gtype not in _unit.PRIMITIVE_TYPES:
      why = 'mesh / height-field geom'
    elif spec['type'] == 'skybox':
      why = 'skybox texture on a geom'
    elif (spec['type'] == '2d') != (gtype == 0):
      why = '2d texture on a solid' if spec['type'] == '2d' else 'cube texture on a plane'
    elif spec['builtin'] == 'none':
      why = 'no builtin pattern'
    elif spec['width'] < 1 or (spec['type'] == '2d' and spec['height'] < 1):
      why = 'texture without a size'
    if why is not None:
      untextured.append(label(g))
      reasons[label(g)] = why
      geoms[g] = None
    elif spec['mark'] == 'random':
      ignored.append(label(g))
  if sky is not None and sky['mark'] == 'random':
    ignored.append('skybox')
  return dict(geoms=geoms, sky=sky, untextured=untextured, reasons=reasons, ignored_marks=ignored)


def _body_id(model, body):
  if body is None:
    return 0
  if isinstance(body, str):
    return model.name2id(body, 'body')
  return int(body)


def resolve_camera(model, cam):
  """One camera in mjModel's terms from a camera name, a camera id, or a user spec -- a dict with the keys
  body (name or id, default world), pos, one of quat | xyaxes | zaxis, fovy (degrees, default 45), mode (one of MODES,
  default 'fixed'), target (body name or id, the targetbody modes).  Returns dict(mode, body, target, pos, quat, fovy,
  pos0, poscom0, mat0, name)."""
  if isinstance(cam, dict):
    unknown = set(cam) - {'body', 'pos', 'quat', 'xyaxes', 'zaxis', 'fovy', 'mode', 'target', 'name'}
    if unknown:
      raise ValueError('unknown camera spec keys: %s' % sorted(unknown))
    if sum(k in cam for k in ('quat', 'xyaxes', 'zaxis')) > 1:
      raise ValueError('a camera spec takes one of quat, xyaxes, zaxis')
    body = _body_id(model, cam.get('body'))
    pos = np.asarray(cam.get('pos', (0, 0, 0)), dtype=np.float64).reshape(3)
    if 'xyaxes' in cam:
      xy = np.asarray(cam['xyaxes'], dtype=np.float64).reshape(6)
      x = xy[:3] / np.linalg.norm(xy[:3])
      y = xy[3:] - x * np.dot(x, xy[3:])
      y /= np.linalg.norm(y)
      quat = mjcf_compiler.mat_to_quat(np.stack([x, y, np.cross(x, y)], 1))
    elif 'zaxis' in cam:
      quat = mjcf_compiler.z_to_quat(np.asarray(cam['zaxis'], dtype=np.float64).reshape(3))
    else:
      quat = np.asarray(cam.get('quat', (1, 0, 0, 0)), dtype=np.float64).reshape(4)
      quat = quat / np.linalg.norm(quat)
    mode = cam.get('mode', 'fixed')
    mode = MODES.index(mode) if isinstance(mode, str) else int(mode)
    target = _body_id(model, cam['target']) if cam.get('target') is not None else -1
    fovy = float(cam.get('fovy', 45.0))
    pos0, poscom0, mat0 = mjcf_compiler.frame_constants(model, [body], [pos], [quat])
    out = dict(mode=mode, body=body, target=target, pos=pos, quat=quat, fovy=fovy, pos0=pos0[0], poscom0=poscom0[0],
               mat0=mat0[0], name=cam.get('name'))
  else:
    i = model.name2id(cam, 'camera') if isinstance(cam, str) else int(cam)
    if not 0 <= i < model.ncam:
      raise ValueError('camera id %d out of range (the model has %d cameras)' % (i, model.ncam))
    consts = mjcf_compiler.camera_constants(model)
    out = dict(mode=int(model.cam_mode[i]), body=int(model.cam_bodyid[i]), target=int(model.cam_targetbodyid[i]),
               pos=np.array(model.cam_pos[i], dtype=np.float64), quat=np.array(model.cam_quat[i], dtype=np.float64),
               fovy=float(model.cam_fovy[i]), pos0=consts[0][i], poscom0=consts[1][i], mat0=consts[2][i],
               name=model.names.get('camera', [None] * model.ncam)[i])
  if not 0 <= out['mode'] < len(MODES):
    raise ValueError('camera mode out of range')
  if out['mode'] >= 3 and out['target'] < 0:
    raise ValueError('a %s camera needs a target body' % MODES[out['mode']])
  if not 0 < out['fovy'] < 180:
    raise ValueError('fovy must lie in (0, 180) degrees')
  return out


def camera_poses(cams, xpos, xmat, subtree_com):
  """World frames of resolved cameras: (pos (B, C, 3), mat (B, C, 3, 3)) from xpos (B, nbody, 3), xmat (B, nbody, 9) and
  subtree_com (B, nbody, 3).  fixed: the body's frame composed with the camera's; track / trackcom: the body origin /
  subtree COM plus the offset at qpos0, orientation fixed at cam_mat0; targetbody / targetbodycom: position as fixed,
  -z through the target's origin / subtree COM, x = normalise(z_world x z_cam), y = z_cam x x."""
  xpos = np.asarray(xpos, dtype=np.float64)
  B = xpos.shape[0]
  xpos = xpos.reshape(B, -1, 3)
  xmat = np.asarray(xmat, dtype=np.float64).reshape(B, -1, 3, 3)
  com = np.asarray(subtree_com, dtype=np.float64).reshape(B, -1, 3)
  pos = np.zeros((B, len(cams), 3))
  mat = np.zeros((B, len(cams), 3, 3))
  for k, c in enumerate(cams):
    b, mode = c['body'], c['mode']
    if mode in (1, 2):
      pos[:, k] = (xpos if mode == 1 else com)[:, b] + (c['pos0'] if mode == 1 else c['poscom0'])
      mat[:, k] = np.asarray(c['mat0']).reshape(3, 3)
      continue
    pos[:, k] = xpos[:, b] + xmat[:, b] @ c['pos']
    if mode == 0:
      mat[:, k] = xmat[:, b] @ mjcf_compiler.quat_to_mat(c['quat']).reshape(3, 3)
      continue
    z = pos[:, k] - (xpos if mode == 3 else com)[:, c['target']]
    n = np.linalg.norm(z, axis=1, keepdims=True)
    z = np.where(n < mjcf_compiler.MINVAL, [0.0, 0, 1], z / np.maximum(n, mjcf_compiler.MINVAL))
    x = np.stack([-z[:, 1], z[:, 0], np.zeros(B)], 1)
    n = np.linalg.norm(x, axis=1, keepdims=True)
    x = np.where(n < mjcf_compiler.MINVAL, [1.0, 0, 0], x / np.maximum(n, mjcf_compiler.MINVAL))
    mat[:, k] = np.stack([x, np.cross(z, x), z], 2)
  return pos, mat


def camera_matrices(cams, pos, mat, height, width):
  """(B, C, 3, 4) camera matrices image @ focal @ rotation @ translation of engine.py:800-808: homogeneous world
  coordinates -> (x, y, w) with pixel = (x / w, y / w)."""
  B, C = pos.shape[:2]
  out = np.zeros((B, C, 3, 4))
  image = np.eye(3)
  image[0, 2] = (width - 1) / 2.0
  image[1, 2] = (height - 1) / 2.0
  for k, c in enumerate(cams):
    f = 0.5 * height / math.tan(math.radians(c['fovy']) / 2)
    focal = np.diag([-f, f, 1.0, 0])[0:3, :]
    for e in range(B):
      tr = np.eye(4)
      tr[0:3, 3] = -pos[e, k]
      rot = np.eye(4)
      rot[0:3, 0:3] = mat[e, k].T
      out[e, k] = image @ focal @ rot @ tr
  return out


class BatchCamera(_unit.BatchUnit):
  """Cameras of every environment of a batch; see the module docstring for what is drawn.

  physics_or_batch: a `BatchedPhysics`, or anything holding one as `.batch` (Physics) or `.physics`.
  cameras: camera names / ids of the model, or user specs (`resolve_camera`).
  """
  _DESTROY = 'dmc_camera_destroy'

  def __init__(self, physics_or_batch, cameras, height, width, near=0.0, far=math.inf, geom_groups=(0, 1, 2), ambient=0.4,
               diffuse=0.6, background=(0, 0, 0), textures=False, texture_filter='nearest', materials=None, skybox=None):
    """textures: draw the model's builtin textures and skybox; materials: {geom name or id: spec} and skybox: spec --
    keys builtin, type, rgb1, rgb2, mark, markrgb, width, height, texrepeat, texuniform, rgba (see `SUITE_GRID`) -- override
    or add to them, and giving either turns textures on; texture_filter: 'nearest' or 'box'."""
    batch = _unit.find_batch(physics_or_batch)
    if batch is None:
      raise TypeError('BatchCamera needs a BatchedPhysics (or an object holding one as .batch / .physics / .host_physics)')
    if isinstance(cameras, (str, int, dict)):
      cameras = [cameras]
    if not cameras:
      raise ValueError('no cameras')
    self.batch, self.model = batch, batch.model
    m = self.model
    self.cameras = [resolve_camera(m, c) for c in cameras]
    self.height, self.width = int(height), int(width)
    self.near, self.far = float(near), float(far)
    self.geom_groups = tuple(int(g) for g in geom_groups)
    self.skipped_geoms = _unit.skipped_geoms(m, 'BatchCamera')
    specs = (_Spec * len(self.cameras))()
    for s, c in zip(specs, self.cameras):
      s.mode, s.bodyid, s.targetbodyid = c['mode'], c['body'], c['target']
      s.pos[:] = list(c['pos'])
      s.mat[:] = list(mjcf_compiler.quat_to_mat(c['quat']).ravel())
      s.pos0[:] = list(c['pos0'])
      s.poscom0[:] = list(c['poscom0'])
      s.mat0[:] = list(np.asarray(c['mat0']).ravel())
      s.fovy = c['fovy']
    self._group = np.ascontiguousarray(m.geom_group, dtype=np.int32)
    self._matid = np.ascontiguousarray(m.geom_matid, dtype=np.int32)
    opt = _Options()
    opt.near_m, opt.far_m, opt.ambient, opt.diffuse = self.near, self.far, float(ambient), float(diffuse)
    opt.background[:] = [float(v) for v in background]
    opt.group_mask = sum(1 << g for g in set(self.geom_groups) if 0 <= g <= 30)
    opt.nmat = int(m.nmat)
    opt.geom_group = self._group.ctypes.data if m.ngeom else None
    opt.geom_matid = self._matid.ctypes.data if m.ngeom else None
    self._ptr = ctypes.c_void_p()
    _native.check(_native.lib().dmc_camera_create(batch._ptr, len(self.cameras), ctypes.cast(specs, ctypes.c_void_p), self.height,
                                                  self.width, ctypes.byref(opt), ctypes.byref(self._ptr)))
    from dm_control_amd.batch import OUT      # pylint: disable=import-outside-toplevel
    self.output_mask = OUT['geom']      # the derived arrays a step launch must write for these cameras
    for c in self.cameras:
      self.output_mask |= {0: OUT['xpos'] | OUT['xmat'], 1: OUT['xpos'], 2: OUT['subtree_com'], 3: OUT['xpos'] | OUT['xmat'],
                           4: OUT['xpos'] | OUT['xmat'] | OUT['subtree_com']}[c['mode']]
    self._colors = None
    self.untextured, self.untextured_reasons, self.ignored_marks = [], {}, []
    self.materials, self.sky = [None] * m.ngeom, None      # what is drawn: per geom a complete spec or None; the skybox spec
    self._tex_request = None
    if textures or materials is not None or skybox is not None:
      self.set_materials(materials, skybox, texture_filter, textures=True)
    elif texture_filter not in FILTERS:
      raise ValueError('texture_filter must be one of %s' % (FILTERS,))
    self.update_colors()

  # -- textures -----------------------------------------------------------------------------------------------------
  def set_materials(self, materials=None, skybox=None, texture_filter='nearest', textures=True):
    """Turns textures on (see __init__) or, with textures=False and nothing else, off again: renders are then the
    flat-colour ones, bit for bit.  Like a colour upload this is synchronous and must not happen inside a graph capture."""
    if texture_filter not in FILTERS:
      raise ValueError('texture_filter must be one of %s' % (FILTERS,))
    if not textures and materials is None and skybox is None:
      self._tex_request = None
      self.untextured, self.untextured_reasons, self.ignored_marks = [], {}, []
      self.materials, self.sky = [None] * self.model.ngeom, None
      _native.check(_native.lib().dmc_camera_set_materials(self._ptr, None, None, 0))
    else:
      self._tex_request = dict(textures=bool(textures), materials=dict(materials) if materials is not None else None,
                               skybox=dict(skybox) if skybox is not None else None, filter=FILTERS.index(texture_filter))
    self._colors = None      # the next update_colors uploads materials and colours
    self.update_colors()

  def clear_materials(self):
    self.set_materials(textures=False)

  def _upload_materials(self):
    req, m = self._tex_request, self.model
    res = resolve_materials(m, req['textures'], req['materials'], req['skybox'])
    self.untextured, self.untextured_reasons, self.ignored_marks = res['untextured'], res['reasons'], res['ignored_marks']
    log = logging.getLogger(__name__)
    if self.untextured:
      log.info('BatchCamera: %d geoms keep their flat colour: %s', len(self.untextured), self.untextured_reasons)
    if self.ignored_marks:
      log.info('BatchCamera: mark="random" is ignored: %s', self.ignored_marks)
    recs = (_Material * max(1, m.ngeom))()
    for g, spec in enumerate(res['geoms']):
      if spec is None:
        continue
      r = recs[g]
      r.mapping = 1 if spec['type'] == '2d' else 2
      r.builtin, r.mark = _DEV_BUILTIN[spec['builtin']], _DEV_MARK[spec['mark']]
      r.width = spec['width']
      r.height = (spec['height'] or spec['width']) if spec['type'] == '2d' else spec['width']
      r.texuniform = int(spec['texuniform'])
      r.rgb1[:], r.rgb2[:], r.markrgb[:], r.texrepeat[:] = spec['rgb1'], spec['rgb2'], spec['markrgb'], spec['texrepeat']
      if spec['rgba'] is not None:
        r.has_rgba = 1
        r.rgba[:] = spec['rgba']
    sky = None
    if res['sky'] is not None:
      sky = _Sky()
      sky.builtin = _DEV_BUILTIN[res['sky']['builtin']]
      sky.rgb1[:], sky.rgb2[:] = res['sky']['rgb1'], res['sky']['rgb2']
    self.materials, self.sky = res['geoms'], res['sky']
    _native.check(_native.lib().dmc_camera_set_materials(self._ptr, ctypes.cast(recs, ctypes.c_void_p),
                                                         ctypes.byref(sky) if sky is not None else None, req['filter']))

  # -- colours ------------------------------------------------------------------------------------------------------
  def update_colors(self, force=False):
    """Uploads the model's geom_rgba / mat_rgba if they changed since the last upload (tasks recolour geoms on the host
    arrays).  `render` calls this; returns whether an upload happened.  The upload is a SYNCHRONOUS copy (it waits for
    the device and is not ordered on the render stream): a render is asynchronous only while the colours are unchanged,
    and colours must not change inside a HIP graph capture -- a captured render keeps drawing the colours uploaded
    before the capture (recolour, call update_colors(), then replay)."""
    m = self.model
    g = np.ascontiguousarray(m.geom_rgba, dtype=np.float64).reshape(-1)
    t = np.ascontiguousarray(m.mat_rgba, dtype=np.float64).reshape(-1)
    key = (g.tobytes(), t.tobytes())
    if self._tex_request is not None and self._tex_request['textures']:      # the model's textures may be recoloured too
      key += tuple(np.ascontiguousarray(getattr(m, k)).tobytes() for k in _TEX_ARRAYS)
    if not force and key == self._colors:
      return False
    if self._tex_request is not None:
      self._upload_materials()      # (before the colours: a record's own rgba takes effect with the colour upload)
    _native.check(_native.lib().dmc_camera_set_colors(self._ptr, g.ctypes.data if g.size else None, t.ctypes.data if t.size else None))
    self._colors = key
    return True

  def set_tuning(self, cull=True, pretransform=True):
    """Tuning studies (scripts/camera_rate.py): the per-tile geom cull and the per-(camera, geom) pre-transform of the
    render kernel, both on by default."""
    _native.check(_native.lib().dmc_camera_set_tuning(self._ptr, int(bool(cull)), int(bool(pretransform))))

  # -- rendering ----------------------------------------------------------------------------------------------------
  def shape(self, kind):
    base = (self.batch.batch_size, len(self.cameras), self.height, self.width)
    return base + {'rgb': (3,), 'depth': (), 'segmentation': (2,)}[kind]

  def _image(self, kind, out=None):
    torch, _, real = self._torch()
    return self._tensor(self.shape(kind), {'rgb': torch.uint8, 'segmentation': torch.int32, 'depth': real}[kind], out)

  def _launch(self, rgb, depth, seg, stream):
    self.update_colors()
    what = (RGB if rgb is not None else 0) | (DEPTH if depth is not None else 0) | (SEG if seg is not None else 0)
    _native.check(_native.lib().dmc_camera_render(self._ptr, what, rgb.data_ptr() if rgb is not None else None,
                                                  depth.data_ptr() if depth is not None else None,
                                                  seg.data_ptr() if seg is not None else None, self.stream_handle(stream)))

  def render(self, depth=False, segmentation=False, out=None, stream=None):
    """One image kind for every (environment, camera): uint8 RGB (B, C, H, W, 3) by default, depth (B, C, H, W) in the
    batch precision, or int32 segmentation (B, C, H, W, 2).  Asynchronous on `stream` (a torch stream or a raw handle;
    default: torch's current stream); `out` is written in place when given."""
    if depth and segmentation:
      raise ValueError('Only one of depth and segmentation can be requested at a time.')      # (engine.py:879-881)
    kind = 'depth' if depth else 'segmentation' if segmentation else 'rgb'
    t = self._image(kind, out)
    self._launch(t if kind == 'rgb' else None, t if kind == 'depth' else None, t if kind == 'segmentation' else None, stream)
    return t

  def render_all(self, stream=None):
    """dict(rgb, depth, segmentation) from ONE launch."""
    out = {k: self._image(k) for k in ('rgb', 'depth', 'segmentation')}
    self._launch(out['rgb'], out['depth'], out['segmentation'], stream)
    return out

  # -- poses --------------------------------------------------------------------------------------------------------
  def poses(self):
    """(pos (B, C, 3), mat (B, C, 3, 3)) from the poses in device memory (a host read: a debugging aid, not a hot path)."""
    b = self.batch
    return camera_poses(self.cameras, b.get('xpos'), b.get('xmat'), b.get('subtree_com'))

  def matrices(self):
    """Per-environment 3x4 camera matrices (B, C, 3, 4) as engine.Camera.matrix builds them (engine.py:800-808)."""
    pos, mat = self.poses()
    return camera_matrices(self.cameras, pos, mat, self.height, self.width)

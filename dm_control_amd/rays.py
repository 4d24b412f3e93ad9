"""BatchRays: mj_ray for a whole batch -- caller-chosen rays and range scans ("lidar"), cast on the device by one HIP launch.

The reference casts one ray of one environment per call (`mujoco.mj_ray`, e.g. locomotion/tasks/random_goal_maze.py:
157-200) and a range scan needs one site and one `<rangefinder>` per ray in the model.  This module gives a batch both as
tensors that never leave the GPU:

  * `cast(pnt, vec)`: arbitrary rays pnt + x vec, (B, R, 3) each; `vec` need not be unit length and x is in units of
    |vec|, as in mj_ray.  Returns the smallest x >= 0 over the geoms that pass the filter and that geom's id; -1 / -1 when
    nothing is hit.
  * `add_scan(frame, directions)` + `scan()`: a fixed table of directions in a frame that moves with the environment -- the
    world, a body, a site, a geom or a fixed model camera -- for every environment in one launch.
  * a geom is skipped when it lies on body `bodyexclude`, is invisible (alpha 0 on the geom or its material: the table the
    rangefinder sensors use), its group's flag in `geomgroup` is zero (groups clamped to 0..5; None: every group),
    `flg_static` is false and its body is welded to the world, or it is a mesh / height field (`skipped_geoms`: scenery
    the rays pass through, as the cameras do).
  * planes are hit from the front only and are finite where their half-sizes are positive; a ray that starts inside a
    closed primitive leaves through its surface.  `cutoff` (metres) turns farther hits into misses.

Poses are the geom_xpos / geom_xmat (and xpos / xmat / site_xpos / site_xmat for a scan's frame) the last step or forward
launch wrote; geom sizes are the ones the step kernel uses (after `set_model_real`, and per environment for
`set_env_geoms` geoms).
"""
import ctypes
import math

import numpy as np

from dm_control_amd import _native
from dm_control_amd import _unit
from dm_control_amd import camera as camera_lib
from dm_control_amd import mjcf_compiler

FRAME_WORLD, FRAME_BODY, FRAME_SITE, FRAME_GEOM = 0, 1, 2, 3
_FRAME_KEYS = {'body': FRAME_BODY, 'site': FRAME_SITE, 'geom': FRAME_GEOM}


class _Options(ctypes.Structure):      # dmc_rays_options
  _fields_ = [('has_geomgroup', ctypes.c_int32), ('flg_static', ctypes.c_int32), ('geomgroup', ctypes.c_int32 * 6),
              ('cutoff', ctypes.c_double), ('geom_group', ctypes.c_void_p), ('ngeom_group', ctypes.c_int32),
              ('reserved', ctypes.c_int32)]


def ring(n_azimuth, elevations=(0.,), fov=2 * math.pi):
  """A direction table (len(elevations) * n_azimuth, 3) of unit vectors, elevation-major: azimuths fov (i + 0.5) /
  n_azimuth - fov / 2 about +z, measured from +x towards +y, at each elevation (radians above the xy plane)."""
  n = int(n_azimuth)
  if n < 1:
    raise ValueError('ring: n_azimuth must be positive')
  el = np.asarray(elevations, dtype=np.float64).reshape(-1)
  if el.size < 1 or not np.all(np.abs(el) <= math.pi / 2):
    raise ValueError('ring: elevations must be a non-empty list of angles in [-pi/2, pi/2]')
  if not 0 < float(fov) <= 2 * math.pi + 1e-12:
    raise ValueError('ring: fov must lie in (0, 2 pi]')
  az = float(fov) * (np.arange(n) + 0.5) / n - float(fov) / 2
  return np.concatenate([np.stack([np.cos(e) * np.cos(az), np.cos(e) * np.sin(az), np.full(n, np.sin(e))], 1) for e in el], 0)


def resolve_frame(model, frame):
  """A scan's frame in the kernel's terms from 'world', dict(body=..), dict(site=..), dict(geom=..) or dict(camera=..)
  (names or ids).  Returns dict(type, id, body, pos (3,), mat (3, 3)): the frame the kernel follows, the body it belongs
  to (-1: the world frame) and a constant pose inside it -- identity except for a camera, whose frame is its body's
  composed with the camera's own (its rays use the camera's axes: -z is the optical axis).  Only fixed cameras have such a
  pose."""
  eye = dict(pos=np.zeros(3), mat=np.eye(3))
  if isinstance(frame, str):
    if frame != 'world':
      raise ValueError("frame: expected 'world' or a dict with one of body / site / geom / camera, got %r" % (frame,))
    return dict(type=FRAME_WORLD, id=0, body=-1, **eye)
  if not isinstance(frame, dict) or len(frame) != 1 or next(iter(frame)) not in ('body', 'site', 'geom', 'camera'):
    raise ValueError("frame: expected 'world' or a dict with one of body / site / geom / camera, got %r" % (frame,))
  kind, key = next(iter(frame.items()))
  if kind == 'camera':
    cam = camera_lib.resolve_camera(model, key)
    if cam['mode'] != 0:
      raise ValueError('frame: a %s camera has no constant pose in a body frame; scans follow fixed cameras only'
                       % camera_lib.MODES[cam['mode']])
    return dict(type=FRAME_BODY, id=cam['body'], body=cam['body'], pos=np.array(cam['pos'], dtype=np.float64),
                mat=mjcf_compiler.quat_to_mat(cam['quat']).reshape(3, 3))
  i = model.name2id(key, kind) if isinstance(key, str) else int(key)
  n = {'body': model.nbody, 'site': model.nsite, 'geom': model.ngeom}[kind]
  if not 0 <= i < n:
    raise ValueError('frame: %s id %d out of range (the model has %d)' % (kind, i, n))
  body = i if kind == 'body' else int(model.site_bodyid[i]) if kind == 'site' else int(model.geom_bodyid[i])
  return dict(type=_FRAME_KEYS[kind], id=i, body=body, **eye)


def resolve_body(model, body):
  """A body id from an id or a name; -1 excludes none."""
  i = model.name2id(body, 'body') if isinstance(body, str) else int(body)
  if not -1 <= i < model.nbody:
    raise ValueError('bodyexclude: body id %d out of range (the model has %d bodies)' % (i, model.nbody))
  return i


def broadcast_rays(pnt, vec, batch_size, dtype=None, device=None):
  """(pnt, vec) as contiguous (B, R, 3) torch tensors from tensors or arrays of shape (B, R, 3), (R, 3) or (3,) each; R is
  taken from whichever argument has it."""
  import torch      # pylint: disable=import-outside-toplevel
  out = []
  for name, a in (('pnt', pnt), ('vec', vec)):
    t = torch.as_tensor(a)
    if dtype is not None or device is not None:
      t = t.to(dtype=dtype or t.dtype, device=device or t.device)
    if t.ndim not in (1, 2, 3) or t.shape[-1] != 3:
      raise ValueError('%s: expected shape (B, R, 3), (R, 3) or (3,), got %s' % (name, tuple(t.shape)))
    if t.ndim == 3 and t.shape[0] != batch_size:
      raise ValueError('%s: the leading axis is %d, the batch holds %d environments' % (name, t.shape[0], batch_size))
    out.append(t.reshape((1,) * (3 - t.ndim) + tuple(t.shape)))
  counts = sorted({t.shape[1] for t in out} - {1})
  if len(counts) > 1:
    raise ValueError('pnt and vec disagree on the number of rays: %s' % counts)
  nray = counts[0] if counts else 1
  return tuple(t.expand(batch_size, nray, 3).contiguous() for t in out)


class BatchRays(_unit.BatchUnit):
  """Ray casts for every environment of a batch; see the module docstring for what is hit.

  physics_or_batch: a `BatchedPhysics`, or anything holding one as `.batch` (Physics) or `.physics`.
  geomgroup: six flags or None (every group); flg_static: False skips the geoms of bodies welded to the world;
  cutoff: metres, farther hits become misses (None: no cutoff).  These are fixed for the object's life.
  """
  _DESTROY = 'dmc_rays_destroy'
  _OUT_ERROR = 'out: expected a contiguous %s tensor of shape %s on %s'

  def __init__(self, physics_or_batch, geomgroup=None, flg_static=True, cutoff=None):
    batch = _unit.find_batch(physics_or_batch)
    if batch is None:
      raise TypeError('BatchRays needs a BatchedPhysics (or an object holding one as .batch / .physics / .host_physics)')
    self.batch, self.model = batch, batch.model
    m = self.model
    opt = _Options()
    if geomgroup is not None:
      flags = [int(bool(v)) for v in np.asarray(geomgroup).reshape(-1)]
      if len(flags) != 6:
        raise ValueError('geomgroup must hold six flags (or be None)')
      opt.has_geomgroup = 1
      opt.geomgroup[:] = flags
    self.geomgroup = None if geomgroup is None else tuple(opt.geomgroup)
    self.flg_static = bool(flg_static)
    if cutoff is not None and not float(cutoff) > 0:
      raise ValueError('cutoff must be positive (or None)')
    self.cutoff = None if cutoff is None or math.isinf(float(cutoff)) else float(cutoff)
    opt.flg_static = int(self.flg_static)
    opt.cutoff = self.cutoff if self.cutoff is not None else 0.0
    self._group = np.ascontiguousarray(m.geom_group, dtype=np.int32)
    opt.geom_group = self._group.ctypes.data if m.ngeom else None
    opt.ngeom_group = int(m.ngeom)
    # the gap, as BatchCamera.untextured states its own: these geoms compile as scenery and no ray hits them
    self.skipped_geoms = _unit.skipped_geoms(m, 'BatchRays')
    self._ptr = ctypes.c_void_p()
    _native.check(_native.lib().dmc_rays_create(batch._ptr, ctypes.byref(opt), ctypes.byref(self._ptr)))
    from dm_control_amd.batch import OUT      # pylint: disable=import-outside-toplevel
    self._OUT = OUT
    self.output_mask = OUT['geom']      # the derived arrays a step launch must write for these rays
    self.scans = []

  def info(self):
    a = np.zeros(8, dtype=np.int32)
    _native.check(_native.lib().dmc_rays_info(self._ptr, a.ctypes.data))
    return dict(zip(('B', 'precision', 'geoms', 'nscan', 'ndir', 'cast_block', 'scan_tile', 'scan_pass'), (int(x) for x in a)))

  # -- tensors ------------------------------------------------------------------------------------------------------
  def _outputs(self, shape, normals, out):
    torch, _, dt = self._torch()
    want = [(shape, dt), (shape, torch.int32)] + ([(shape + (3,), dt)] if normals else [])
    out = [None] * len(want) if out is None else list(out)
    if len(out) != len(want):
      raise ValueError('out must hold %d tensors (dist, geomid%s)' % (len(want), ', normal' if normals else ''))
    return [self._tensor(s, d, o) for (s, d), o in zip(want, out)]

  # -- arbitrary rays -----------------------------------------------------------------------------------------------
  def cast(self, pnt, vec, bodyexclude=-1, normals=False, out=None, stream=None):
    """mj_ray for R rays of every environment in one launch.  pnt, vec: (B, R, 3) torch tensors; (R, 3) and (3,) broadcast.
    bodyexclude: a body id or name, or an int tensor (B,) / (B, R) of ids (-1: none).  Returns (dist (B, R) in the batch
    precision, -1 on a miss; geomid (B, R) int32[; normal (B, R, 3): the world-frame unit normal at the hit]).  Asynchronous
    on `stream` (a torch stream or a raw handle; default: torch's current stream); `out`, a sequence of such tensors, is
    written in place."""
    torch, dev, dt = self._torch()
    B = self.batch.batch_size
    p, v = broadcast_rays(pnt, vec, B, dt, dev)
    R = p.shape[1]
    bex, bex_t, per_ray = -1, None, 0
    if isinstance(bodyexclude, torch.Tensor):
      if tuple(bodyexclude.shape) not in ((B,), (B, R)):
        raise ValueError('bodyexclude: a tensor must have shape (B,) = %s or (B, R) = %s' % ((B,), (B, R)))
      bex_t = bodyexclude.to(device=dev, dtype=torch.int32).contiguous()
      per_ray = int(bex_t.ndim == 2)
    else:
      bex = resolve_body(self.model, bodyexclude)
    res = self._outputs((B, R), normals, out)
    _native.check(_native.lib().dmc_rays_cast(self._ptr, R, p.data_ptr(), v.data_ptr(), bex,
                                              bex_t.data_ptr() if bex_t is not None else None, per_ray, res[0].data_ptr(),
                                              res[1].data_ptr(), res[2].data_ptr() if normals else None,
                                              self.stream_handle(stream)))
    return tuple(res)

  # -- scans --------------------------------------------------------------------------------------------------------
  def add_scan(self, frame, directions, offset=(0, 0, 0), bodyexclude='frame'):
    """Adds a scan: `directions` (R, 3) in `frame` ('world', dict(body=..), dict(site=..), dict(geom=..), dict(camera=..)),
    cast from `offset` in that frame.  bodyexclude: 'frame' = the body the frame belongs to, as a rangefinder skips its
    site's body (none for the world frame), or a body id / name, -1 for none.  Every scan of one object has the same R.
    Uploads tables: not inside a graph capture.  Returns the scan's index."""
    f = resolve_frame(self.model, frame)
    d = np.asarray(directions, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 3 or d.shape[0] < 1 or not np.all(np.isfinite(d)):
      raise ValueError('directions: expected a finite (R, 3) array')
    if self.scans and d.shape[0] != self.scans[0]['directions'].shape[0]:
      raise ValueError('every scan of one BatchRays has the same number of directions (%d)' % self.scans[0]['directions'].shape[0])
    off = np.asarray(offset, dtype=np.float64).reshape(3)
    bex = f['body'] if isinstance(bodyexclude, str) and bodyexclude == 'frame' else resolve_body(self.model, bodyexclude)
    # a camera's constant pose inside its body folds into the tables: the kernel follows the body
    dirs = np.ascontiguousarray(d @ f['mat'].T)
    origin = np.ascontiguousarray(f['pos'] + f['mat'] @ off)
    _native.check(_native.lib().dmc_rays_add_scan(self._ptr, f['type'], f['id'], origin.ctypes.data, bex, dirs.shape[0], dirs.ctypes.data))
    OUT = self._OUT
    self.output_mask |= {FRAME_WORLD: 0, FRAME_BODY: OUT['xpos'] | OUT['xmat'], FRAME_SITE: OUT['site'], FRAME_GEOM: 0}[f['type']]
    self.scans.append(dict(frame=f, directions=d.copy(), offset=off, bodyexclude=bex, local_dirs=dirs, local_origin=origin))
    return len(self.scans) - 1

  def scan(self, normals=False, out=None, stream=None):
    """Every scan of every environment in one launch: (dist (B, nscan, R), geomid (B, nscan, R)[, normal (B, nscan, R, 3)]);
    dist is in units of the direction's length (metres for unit directions)."""
    if not self.scans:
      raise ValueError('no scan was added (add_scan)')
    shape = (self.batch.batch_size, len(self.scans), self.scans[0]['directions'].shape[0])
    res = self._outputs(shape, normals, out)
    _native.check(_native.lib().dmc_rays_scan(self._ptr, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr() if normals else None,
                                              self.stream_handle(stream)))
    return tuple(res)

  def scan_rays(self, k, xpos, xmat, site_xpos, site_xmat, geom_xpos, geom_xmat):
    """World-frame (pnt (3,), vec (R, 3)) of scan k for one environment from its poses read back to the host (a debugging
    aid, not a hot path): xpos (nbody, 3), xmat (nbody, 9), ... as `batch.get` returns them per environment."""
    s = self.scans[k]
    f = s['frame']
    if f['type'] == FRAME_WORLD:
      return s['local_origin'].copy(), s['local_dirs'].copy()
    pos, mat = {FRAME_BODY: (xpos, xmat), FRAME_SITE: (site_xpos, site_xmat), FRAME_GEOM: (geom_xpos, geom_xmat)}[f['type']]
    R = np.asarray(mat, dtype=np.float64).reshape(-1, 3, 3)[f['id']]
    return np.asarray(pos, dtype=np.float64).reshape(-1, 3)[f['id']] + R @ s['local_origin'], s['local_dirs'] @ R.T

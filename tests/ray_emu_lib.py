"""TEST INFRASTRUCTURE: host build of the ray unit's per-ray functions, see tests/emu/ray_emu.cpp."""
import ctypes
import os

import numpy as np

import host_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, 'emu', 'ray_emu.cpp')
_lib = None


def lib():
  global _lib
  if _lib is None:
    L = host_build.load(_SRC, 'ray_emu')
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.ray_emu_cast.argtypes = [ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, cd, vp, vp, vp]
    L.ray_emu_cast.restype = None
    L.ray_emu_scan.argtypes = [ci, ci, vp, vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, cd, vp, vp]
    L.ray_emu_scan.restype = None
    L.ray_emu_step.argtypes = [ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ray_emu_step.restype = None
    _lib = L
  return _lib


_c64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
_i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)


def _geoms(model, hittable, geom_xpos, geom_xmat, geom_size):
  size = _c64(model.geom_size if geom_size is None else geom_size)
  return model.ngeom, _i32(model.geom_type), _i32(model.geom_bodyid), _i32(~np.asarray(hittable, dtype=bool)), size, _c64(geom_xpos), _c64(geom_xmat)


def cast(prec, model, hittable, geom_xpos, geom_xmat, pnt, vec, bodyexclude=-1, cutoff=None, geom_size=None, step=False):
  """The cast kernel's walk on the host in fp32 / fp64 (step=True: the step kernel's ray_geom_any instead, fp64, no cutoff
  and no normals).  Returns (dist (N), gid (N), normal (N, 3))."""
  pnt, vec = _c64(pnt).reshape(-1, 3), _c64(vec).reshape(-1, 3)
  n = len(vec)
  bex = _i32(np.broadcast_to(np.asarray(bodyexclude), (n,)))
  ng, typ, body, skip, size, gp, gm = _geoms(model, hittable, geom_xpos, geom_xmat, geom_size)
  dist, gid, normal = np.zeros(n), np.zeros(n, np.int32), np.zeros((n, 3))
  if step:
    lib().ray_emu_step(n, pnt.ctypes.data, vec.ctypes.data, bex.ctypes.data, ng, typ.ctypes.data, body.ctypes.data, skip.ctypes.data,
                       size.ctypes.data, gp.ctypes.data, gm.ctypes.data, dist.ctypes.data, gid.ctypes.data)
  else:
    lib().ray_emu_cast(prec, n, pnt.ctypes.data, vec.ctypes.data, bex.ctypes.data, ng, typ.ctypes.data, body.ctypes.data,
                       skip.ctypes.data, size.ctypes.data, gp.ctypes.data, gm.ctypes.data, np.inf if cutoff is None else cutoff,
                       dist.ctypes.data, gid.ctypes.data, normal.ctypes.data)
  return dist, gid, normal


def scan(prec, model, hittable, geom_xpos, geom_xmat, frame_type, frame_pos, frame_mat, offset, dirs, bodyexclude=-1, cutoff=None,
         geom_size=None):
  """The scan kernel's walk on the host: (dist (N), gid (N)) of frame-local directions."""
  dirs = _c64(dirs).reshape(-1, 3)
  n = len(dirs)
  fp, fm, off = _c64(frame_pos).reshape(3), _c64(frame_mat).reshape(9), _c64(offset).reshape(3)
  ng, typ, body, skip, size, gp, gm = _geoms(model, hittable, geom_xpos, geom_xmat, geom_size)
  dist, gid = np.zeros(n), np.zeros(n, np.int32)
  lib().ray_emu_scan(prec, frame_type, fp.ctypes.data, fm.ctypes.data, off.ctypes.data, int(bodyexclude), n, dirs.ctypes.data, ng,
                     typ.ctypes.data, body.ctypes.data, skip.ctypes.data, size.ctypes.data, gp.ctypes.data, gm.ctypes.data,
                     np.inf if cutoff is None else cutoff, dist.ctypes.data, gid.ctypes.data)
  return dist, gid

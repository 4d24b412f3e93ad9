"""TEST INFRASTRUCTURE: host build of the camera's device functions, see tests/emu/camera_emu.cpp."""
import ctypes
import os

import numpy as np

import host_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, 'emu', 'camera_emu.cpp')
_lib = None


def lib():
  global _lib
  if _lib is None:
    L = host_build.load(_SRC, 'camera_emu')
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.cam_emu_render.argtypes = [ci, vp, vp, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, cd, cd, cd, cd, vp, vp, vp]
    L.cam_emu_render.restype = None
    L.cam_emu_pose.argtypes = [ci, ci, ci] + [vp] * 10
    L.cam_emu_pose.restype = None
    _lib = L
  return _lib


def render(prec, cam_pos, cam_mat, fovy, H, W, geom_type, geom_size, geom_xpos, geom_xmat, visible, color, near=0.0,
           far=np.inf, ambient=0.4, diffuse=0.6):
  """The signature of camera_twin.render; returns (depth, gid, rgb)."""
  n = len(geom_type)
  c64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
  pos, mat, size, gp, gm = c64(cam_pos), c64(cam_mat), c64(geom_size), c64(geom_xpos), c64(geom_xmat)
  typ = np.ascontiguousarray(geom_type, dtype=np.int32)
  skip = np.ascontiguousarray(~np.asarray(visible, dtype=bool), dtype=np.int32)
  col = np.ascontiguousarray(color, dtype=np.float32)
  depth, gid, rgb = np.zeros((H, W)), np.zeros((H, W), np.int32), np.zeros((H, W, 3), np.uint8)
  lib().cam_emu_render(prec, pos.ctypes.data, mat.ctypes.data, fovy, H, W, n, typ.ctypes.data, skip.ctypes.data,
                       size.ctypes.data, gp.ctypes.data, gm.ctypes.data, col.ctypes.data, near, far, ambient, diffuse,
                       depth.ctypes.data, gid.ctypes.data, rgb.ctypes.data)
  return depth, gid, rgb


def pose(cam, xpos, xmat, com):
  """(pos (3,), mat (3, 3)) of a resolved camera (camera.resolve_camera) for one environment."""
  from dm_control_amd import mjcf_compiler
  c64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
  a = [c64(cam['pos']), c64(mjcf_compiler.quat_to_mat(cam['quat'])), c64(cam['pos0']), c64(cam['poscom0']), c64(cam['mat0']),
       c64(xpos), c64(xmat), c64(com)]
  op, om = np.zeros(3), np.zeros(9)
  lib().cam_emu_pose(cam['mode'], cam['body'], cam['target'], *[x.ctypes.data for x in a], op.ctypes.data, om.ctypes.data)
  return op, om.reshape(3, 3)

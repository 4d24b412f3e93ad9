"""TEST INFRASTRUCTURE: host build of the camera's texture functions, see tests/emu/camera_texture_emu.cpp."""
import ctypes
import os

import numpy as np

import host_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, 'emu', 'camera_texture_emu.cpp')
_lib = None
BUILTIN = {'flat': 0, 'checker': 1, 'gradient': 2}
MARK = {'none': 0, 'random': 0, 'edge': 1, 'cross': 2}


def lib():
  global _lib
  if _lib is None:
    L = host_build.load(_SRC, 'camera_texture_emu')
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.cam_tex_emu_render.argtypes = [ci, vp, vp, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, cd, cd, cd, cd, vp, vp, vp]
    L.cam_tex_emu_render.restype = None
    L.cam_tex_emu_texel.argtypes = [vp, vp, cd, cd, vp]
    L.cam_tex_emu_texel.restype = None
    L.cam_tex_emu_box.argtypes = [ci, vp, vp, cd, cd, cd, cd, vp]
    L.cam_tex_emu_box.restype = None
    L.cam_tex_emu_cube.argtypes = [vp, vp, ci, vp, vp, vp]
    L.cam_tex_emu_cube.restype = ci
    L.cam_tex_emu_sky.argtypes = [vp, vp, ci, vp, cd, cd, vp]
    L.cam_tex_emu_sky.restype = None
    _lib = L
  return _lib


def pack(specs):
  """(mi (n, 6) int32, md (n, 11) float64) from complete material specs (camera.material_spec) or None per geom."""
  mi, md = np.zeros((len(specs), 6), np.int32), np.zeros((len(specs), 11))
  for g, s in enumerate(specs):
    if s is None:
      continue
    two_d = s['type'] == '2d'
    mi[g] = [1 if two_d else 2, BUILTIN[s['builtin']], MARK[s['mark']], s['width'], (s['height'] or s['width']) if two_d else s['width'],
             int(s['texuniform'])]
    md[g] = list(s['texrepeat']) + list(s['rgb1']) + list(s['rgb2']) + list(s['markrgb'])
  return mi, md


def texel(spec, u, v):
  mi, md = pack([spec])
  out = np.zeros(3, np.float32)
  lib().cam_tex_emu_texel(mi.ctypes.data, md.ctypes.data, u, v, out.ctypes.data)
  return out.astype(np.float64)


def box(spec, u, v, hu, hv, prec=64):
  mi, md = pack([spec])
  out = np.zeros(3, np.float32)
  lib().cam_tex_emu_box(prec, mi.ctypes.data, md.ctypes.data, u, v, hu, hv, out.ctypes.data)
  return out.astype(np.float64)


def cube(spec, gtype, size, p):
  mi, md = pack([spec])
  size, p, uv = np.ascontiguousarray(size, dtype=np.float64), np.ascontiguousarray(p, dtype=np.float64), np.zeros(2)
  face = lib().cam_tex_emu_cube(mi.ctypes.data, md.ctypes.data, gtype, size.ctypes.data, p.ctypes.data, uv.ctypes.data)
  return face, uv


def sky(spec, R, dx, dy):
  a, b = np.asarray(spec['rgb1'], np.float32), np.asarray(spec['rgb2'], np.float32)
  R = np.ascontiguousarray(R, dtype=np.float64)
  out = np.zeros(3, np.uint8)
  lib().cam_tex_emu_sky(a.ctypes.data, b.ctypes.data, BUILTIN[spec['builtin']], R.ctypes.data, dx, dy, out.ctypes.data)
  return out


def render(prec, cam_pos, cam_mat, fovy, H, W, geom_type, geom_size, geom_xpos, geom_xmat, visible, color, specs, sky_spec=None,
           texture_filter='nearest', near=0.0, far=np.inf, ambient=0.4, diffuse=0.6):
  """camera_texture_twin.render's arguments; returns (depth, gid, rgb)."""
  n = len(geom_type)
  c64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
  pos, mat, size, gp, gm = c64(cam_pos), c64(cam_mat), c64(geom_size), c64(geom_xpos), c64(geom_xmat)
  typ = np.ascontiguousarray(geom_type, dtype=np.int32)
  skip = np.ascontiguousarray(~np.asarray(visible, dtype=bool), dtype=np.int32)
  col = np.ascontiguousarray(color, dtype=np.float32)
  mi, md = pack(specs)
  s1 = np.asarray(sky_spec['rgb1'] if sky_spec else (0, 0, 0), np.float32)
  s2 = np.asarray(sky_spec['rgb2'] if sky_spec else (0, 0, 0), np.float32)
  sky_on = 1 + BUILTIN[sky_spec['builtin']] if sky_spec else 0
  depth, gid, rgb = np.zeros((H, W)), np.zeros((H, W), np.int32), np.zeros((H, W, 3), np.uint8)
  lib().cam_tex_emu_render(prec, pos.ctypes.data, mat.ctypes.data, fovy, H, W, n, typ.ctypes.data, skip.ctypes.data,
                           size.ctypes.data, gp.ctypes.data, gm.ctypes.data, col.ctypes.data, mi.ctypes.data, md.ctypes.data,
                           ('nearest', 'box').index(texture_filter), sky_on, s1.ctypes.data, s2.ctypes.data, near, far, ambient, diffuse,
                           depth.ctypes.data, gid.ctypes.data, rgb.ctypes.data)
  return depth, gid, rgb

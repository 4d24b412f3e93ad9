"""TEST INFRASTRUCTURE: host build of the distance unit's per-pair solver, see tests/emu/dist_emu.cpp."""
import ctypes
import os

import numpy as np

import host_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, 'emu', 'dist_emu.cpp')
_lib = None


def lib():
  global _lib
  if _lib is None:
    L = host_build.load(_SRC, 'dist_emu')
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.dist_emu_pairs.argtypes = [ci, ci, vp, vp, vp, vp, vp, cd, ci, vp]
    L.dist_emu_pairs.restype = None
    L.dist_emu_caps.argtypes = [vp]
    L.dist_emu_caps.restype = None
    _lib = L
  return _lib


def caps():
  a = np.zeros(7, np.int32)
  lib().dist_emu_caps(a.ctypes.data)
  return dict(zip(('V32', 'F32', 'V64', 'F64', 'block', 'K32', 'K64'), (int(v) for v in a)))


def pairs(prec, geoms1, geoms2, distmax=10.0, tolerance=1e-6, iterations=50):
  """The solver on n pairs of twin-style geoms (objects with type, size, pos, mat): dict(dist (n), fromto (n, 6),
  normal (n, 3), status (n), epa (n), gap (n): the gap the solver certified)."""
  n = len(geoms1)
  typ = np.array([[a.type, b.type] for a, b in zip(geoms1, geoms2)], dtype=np.int32)
  pack = lambda f, k: np.ascontiguousarray([[np.asarray(f(a), dtype=np.float64).reshape(k), np.asarray(f(b), dtype=np.float64).reshape(k)]
                                            for a, b in zip(geoms1, geoms2)], dtype=np.float64)
  size, pos, mat = pack(lambda g: g.size, 3), pack(lambda g: g.pos, 3), pack(lambda g: g.mat, 9)
  dm = np.ascontiguousarray(np.broadcast_to(np.asarray(distmax, dtype=np.float64), (n,)))
  out = np.zeros((n, 13))
  lib().dist_emu_pairs(int(prec), n, typ.ctypes.data, size.ctypes.data, pos.ctypes.data, mat.ctypes.data, dm.ctypes.data,
                       float(tolerance), int(iterations), out.ctypes.data)
  return dict(dist=out[:, 0], fromto=out[:, 1:7].copy(), normal=out[:, 7:10].copy(), status=out[:, 10].astype(np.int32),
              epa=out[:, 11].astype(np.int32), gap=out[:, 12].copy())

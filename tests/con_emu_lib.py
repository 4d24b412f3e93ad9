"""TEST INFRASTRUCTURE: host build of the contact-wrench unit's core, see tests/emu/con_emu.cpp."""
import ctypes
import os

import numpy as np

import host_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, 'emu', 'con_emu.cpp')
_lib = None
FIELDS = ('ncon', 'geom1', 'geom2', 'dist', 'pos', 'frame', 'force', 'xpos', 'xipos', 'xmat')


def lib():
  global _lib
  if _lib is None:
    L = host_build.load(_SRC, 'con_emu')
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.con_emu_run.argtypes = [ci]*5 + [vp]*10 + [ci, ci, vp, vp, ci, ci] + [vp]*6
    L.con_emu_run.restype = None
    L.con_emu_caps.argtypes = [ci, vp]
    L.con_emu_caps.restype = None
    _lib = L
  return _lib


def caps(ngeom=1):
  a = np.zeros(5, np.int32)
  lib().con_emu_caps(int(ngeom), a.ctypes.data)
  return dict(zip(('block', 'max_targets', 'max_words', 'head', 'words'), (int(v) for v in a)))


def run(prec, arrays, tables, ngeom, nbody, local=False, what=('wrench', 'force', 'torque', 'normal', 'count', 'dist')):
  """The unit's outputs for B environments from the host build: dict(wrench (B, K, 6), force, torque (B, T, 3), normal,
  dist (B, T), count (B, T) int32), prefilled with NaN / -1 so that an element the core leaves out shows.  arrays: dict of
  FIELDS, environment-major ((B,), (B, K), (B, K, 3), (B, K, 3, 3), (B, K, 6), (B, nbody, 3), .., (B, nbody, 3, 3));
  tables: contacts.target_tables(model, targets, about)."""
  n = np.ascontiguousarray(arrays['ncon'], dtype=np.int32).reshape(-1)
  B = n.size
  g1, g2 = (np.ascontiguousarray(arrays[k], dtype=np.int32).reshape(B, -1) for k in ('geom1', 'geom2'))
  K = g1.shape[1]
  f64 = lambda k, *s: np.ascontiguousarray(arrays[k], dtype=np.float64).reshape((B,) + s)
  dist, pos, frame, force = f64('dist', K), f64('pos', K, 3), f64('frame', K, 9), f64('force', K, 6)
  xpos, xipos, xmat = f64('xpos', nbody, 3), f64('xipos', nbody, 3), f64('xmat', nbody, 9)
  body, masks = tables['body'], tables['masks']
  T, words = masks.shape[0], masks.shape[2]
  out = dict(wrench=np.full((B, K, 6), np.nan), force=np.full((B, T, 3), np.nan), torque=np.full((B, T, 3), np.nan),
             normal=np.full((B, T), np.nan), count=np.full((B, T), -1, dtype=np.int32), dist=np.full((B, T), np.nan))
  ptr = lambda k: out[k].ctypes.data if k in what else None
  lib().con_emu_run(int(prec), B, K, int(ngeom), int(nbody), n.ctypes.data, g1.ctypes.data, g2.ctypes.data, dist.ctypes.data,
                    pos.ctypes.data, frame.ctypes.data, force.ctypes.data, xpos.ctypes.data, xipos.ctypes.data, xmat.ctypes.data,
                    T, words, body.ctypes.data, masks.ctypes.data, int(tables['about']), int(bool(local)),
                    ptr('wrench'), ptr('force'), ptr('torque'), ptr('normal'), ptr('count'), ptr('dist'))
  return {k: out[k] for k in what}

"""TEST INFRASTRUCTURE: host build of the Jacobian unit's core, see tests/emu/jac_emu.cpp."""
import ctypes
import os

import numpy as np

import host_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, 'emu', 'jac_emu.cpp')
_lib = None


def lib():
  global _lib
  if _lib is None:
    L = host_build.load(_SRC, 'jac_emu')
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.jac_emu_run.argtypes = [ci, ci, ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp]
    L.jac_emu_run.restype = None
    L.jac_emu_sincos.argtypes = [ci, ci, vp, vp, vp]
    L.jac_emu_sincos.restype = None
    L.jac_emu_caps.argtypes = [vp]
    L.jac_emu_caps.restype = None
    _lib = L
  return _lib


def caps():
  a = np.zeros(3, np.int32)
  lib().jac_emu_caps(a.ctypes.data)
  return dict(zip(('max_chain_dofs', 'block', 'head'), (int(v) for v in a)))


def sincos(prec, x):
  x = np.ascontiguousarray(x, dtype=np.float64)
  s, c = np.zeros_like(x), np.zeros_like(x)
  lib().jac_emu_sincos(int(prec), x.size, x.ctypes.data, s.ctypes.data, c.ctypes.data)
  return s, c


def run(prec, tables, qpos, qvel, point=None, force=None, torque=None, local=False):
  """One environment through the unit's three launches: dict(jacp, jacr (T, 3, C), vel (T, 6), qfrc (C)).  tables:
  jacobian.chain_tables(...); point / force / torque: (T, 3) or None."""
  T, C = len(tables['dims']), len(tables['columns'])
  f64 = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (T, 3)))
  qpos, qvel = np.ascontiguousarray(qpos, dtype=np.float64), np.ascontiguousarray(qvel, dtype=np.float64)
  point, force, torque = f64(point), f64(force), f64(torque)
  ptr = lambda a: None if a is None else a.ctypes.data
  jacp, jacr, vel, qfrc = np.zeros((T, 3, C)), np.zeros((T, 3, C)), np.zeros((T, 6)), np.zeros(C)
  lib().jac_emu_run(int(prec), T, C, tables['dims'].ctypes.data, tables['ints'].ctypes.data, tables['reals'].ctypes.data,
                    tables['reals'].size, qpos.size, qvel.size, qpos.ctypes.data, qvel.ctypes.data, ptr(point), ptr(force), ptr(torque),
                    int(bool(local)), jacp.ctypes.data, jacr.ctypes.data, vel.ctypes.data, qfrc.ctypes.data)
  return dict(jacp=jacp, jacr=jacr, vel=vel, qfrc=qfrc)

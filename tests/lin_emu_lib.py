"""TEST INFRASTRUCTURE: host build of the linearisation unit's core, see tests/emu/lin_emu.cpp."""
import ctypes
import os

import numpy as np

import host_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, 'emu', 'lin_emu.cpp')
_lib = None
FAN_FIELDS = ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart', 'qfrc_applied', 'xfrc_applied', 'mocap_pos', 'mocap_quat', 'time')
STEPPED_FIELDS = ('qpos', 'qvel', 'act', 'sensordata')


def lib():
  global _lib
  if _lib is None:
    L = host_build.load(_SRC, 'lin_emu')
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.lin_emu_sizes.argtypes = [vp, vp]
    L.lin_emu_fan.argtypes = [ci, vp, vp, vp, cd, vp, vp, vp]
    L.lin_emu_diff.argtypes = [ci, vp, vp, vp, cd, vp, vp, ci, vp, vp, vp, vp]
    L.lin_emu_sub_quat.argtypes = [ci, vp, vp, vp]
    for f in (L.lin_emu_sizes, L.lin_emu_fan, L.lin_emu_diff, L.lin_emu_sub_quat):
      f.restype = None
    _lib = L
  return _lib


def dims_array(model, centered=True, xfrc=False):
  m = model
  return np.array([m.njnt, m.nq, m.nv, m.na, m.nu, m.nbody, getattr(m, 'nmocap', 0), m.nsensordata, int(xfrc), int(centered)],
                  dtype=np.int32)


def sizes(dims):
  a = np.zeros(8, np.int32)
  lib().lin_emu_sizes(dims.ctypes.data, a.ctypes.data)
  return dict(zip(('P', 'nx', 'nin', 'fan_reals', 'stepped_reals', 'nints', 'nreals', 'block'), (int(v) for v in a)))


def field_rows(model, xfrc=False):
  m = model
  nm = int(getattr(m, 'nmocap', 0))
  return dict(qpos=m.nq, qvel=m.nv, act=m.na, ctrl=m.nu, qacc_warmstart=m.nv, qfrc_applied=m.nv, xfrc_applied=6 * m.nbody if xfrc else 0,
              mocap_pos=3 * nm, mocap_quat=4 * nm, time=1, sensordata=m.nsensordata)


def fan(prec, model, tables, eps, nominal, centered=True, xfrc=False):
  """One environment's nominal inputs `nominal` ({field: array}; missing fields are zeros) through the fan-out:
  ({field: (P, rows)}, flags (nu,))."""
  dims = dims_array(model, centered, xfrc)
  sz = sizes(dims)
  rows = field_rows(model, xfrc)
  flat = np.concatenate([np.asarray(nominal.get(f, np.zeros(rows[f])), dtype=np.float64).reshape(-1)[:rows[f]] if rows[f] else np.zeros(0)
                         for f in FAN_FIELDS])
  assert flat.size == sz['fan_reals'], (flat.size, sz)
  cols = np.full((sz['P'], sz['fan_reals']), np.nan)
  flags = np.full(max(1, model.nu), -1, np.int32)
  lib().lin_emu_fan(int(prec), dims.ctypes.data, tables['ints'].ctypes.data, tables['reals'].ctypes.data, float(eps), flat.ctypes.data,
                    cols.ctypes.data, flags.ctypes.data)
  out, at = {}, 0
  for f in FAN_FIELDS:
    out[f] = cols[:, at:at + rows[f]].copy()
    at += rows[f]
  return out, flags[:model.nu].copy()


def diff(prec, model, tables, eps, stepped, flags, centered=True, sensors=True):
  """The stepped columns `stepped` ({qpos, qvel, act, sensordata: (P, rows)}) through the difference: (A, B, C, D)."""
  m = model
  dims = dims_array(m, centered)
  sz = sizes(dims)
  P, nx, nu, ns = sz['P'], sz['nx'], m.nu, m.nsensordata
  cols = np.ascontiguousarray(np.concatenate([np.asarray(stepped[f], dtype=np.float64).reshape(P, -1) for f in STEPPED_FIELDS], axis=1))
  assert cols.shape == (P, sz['stepped_reals']), (cols.shape, sz)
  A, B, C, D = (np.full(s, np.nan) for s in ((nx, nx), (nx, nu), (ns, nx), (ns, nu)))
  fl = np.ascontiguousarray(np.concatenate([np.asarray(flags, dtype=np.int32).reshape(-1), np.zeros(1, np.int32)]))
  lib().lin_emu_diff(int(prec), dims.ctypes.data, tables['ints'].ctypes.data, tables['reals'].ctypes.data, float(eps), cols.ctypes.data,
                     fl.ctypes.data, int(bool(sensors)), A.ctypes.data, B.ctypes.data, C.ctypes.data, D.ctypes.data)
  return A, B, C, D


def sub_quat(prec, qa, qb):
  qa, qb = (np.ascontiguousarray(q, dtype=np.float64) for q in (qa, qb))
  res = np.zeros(3)
  lib().lin_emu_sub_quat(int(prec), qa.ctypes.data, qb.ctypes.data, res.ctypes.data)
  return res

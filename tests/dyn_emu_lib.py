"""TEST INFRASTRUCTURE: host build of the dynamics unit's core, see tests/emu/dyn_emu.cpp."""
import ctypes
import os

import numpy as np

import host_build

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, 'emu', 'dyn_emu.cpp')
_lib = None
_WHAT = dict(M=1, bias=2, inverse=4, mul=8, solve=16)


def lib():
  global _lib
  if _lib is None:
    L = host_build.load(_SRC, 'dyn_emu')
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.dyn_emu_run.argtypes = [ci, vp, vp, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.dyn_emu_run.restype = None
    L.dyn_emu_caps.argtypes = [ci, ci, ci, vp]
    L.dyn_emu_caps.restype = None
    _lib = L
  return _lib


def caps(nb=2, nv=1, lanes=64):
  a = np.zeros(9, np.int32)
  lib().dyn_emu_caps(int(nb), int(nv), int(lanes), a.ctypes.data)
  return dict(zip(('max_dofs', 'block', 'chunk', 'ws0', 'ws1', 'tier64', 'tier32', 'nints0', 'nreals0'), (int(v) for v in a)))


def dims_array(tables):
  d = tables['dims']
  return np.array([d[k] for k in ('nb', 'nj', 'nv', 'nq', 'nlevel', 'nsub')], dtype=np.int32)


def run(prec, tables, qpos, qvel=None, qacc=None, vec=None, lanes=64, what=None):
  """One environment through the unit's calls: dict(M (nv, nv), bias (nv), inverse (nv), mul, solve (K, nv)) -- M and bias
  always, inverse with `qacc`, mul and solve with `vec` (K, nv) or (nv,); `what`: a subset of those names.  tables:
  dynamics.model_tables(model)."""
  d = tables['dims']
  nv = d['nv']
  f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
  qpos = f64(qpos)
  qvel = np.zeros(nv) if qvel is None else f64(qvel)
  assert qpos.shape == (d['nq'],) and qvel.shape == (nv,)
  names = ['M', 'bias'] + (['inverse'] if qacc is not None else []) + (['mul', 'solve'] if vec is not None else [])
  names = [n for n in names if what is None or n in what]
  qacc = np.zeros(nv) if qacc is None else f64(qacc)
  flat = vec is not None and np.ndim(vec) == 1
  vec = np.zeros((1, nv)) if vec is None else f64(np.reshape(vec, (-1, nv)))
  K = vec.shape[0]
  M, bias, inv, mul, sol = np.zeros((nv, nv)), np.zeros(nv), np.zeros(nv), np.zeros((K, nv)), np.zeros((K, nv))
  dims = dims_array(tables)
  lib().dyn_emu_run(int(prec), dims.ctypes.data, tables['ints'].ctypes.data, tables['reals'].ctypes.data, int(lanes),
                    sum(_WHAT[n] for n in names), qpos.ctypes.data, qvel.ctypes.data, qacc.ctypes.data, K, vec.ctypes.data,
                    M.ctypes.data, bias.ctypes.data, inv.ctypes.data, mul.ctypes.data, sol.ctypes.data)
  out = dict(M=M, bias=bias, inverse=inv, mul=mul[0] if flat else mul, solve=sol[0] if flat else sol)
  return {k: out[k] for k in names}

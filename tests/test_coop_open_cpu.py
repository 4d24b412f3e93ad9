"""The cooperative opening stage (csrc/step_core.h: coop_side_a / coop_side_b) on the host build of the kernel core.  No GPU.

On stashed kinematics the opening stage of a step is two sides -- A: mass matrix, its factor, bias and passive forces; B:
contacts and constraint rows -- that two waves of a workgroup run at the same time.  The licence for that is that neither
side reads what the other writes.  Here the sides run one after the other in BOTH orders from one state of the
environment's scratch, and the whole scratch (every real and every int array, overlays included) must come out the same
bits as after the stage as one wave runs it (stage_posvel).  The check that covers every model is reading the layout
(csrc/step_layout.h); this one shows it for the small suite models and the model with every joint type.

The host build has one lane per environment, so the 16-lane instantiation of the sides against the 32-lane stage is not
compared here: tests/test_gpu_coop_open.py does that on the device, bit for bit.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from dm_control_amd import mjcf_compiler as mc
from dm_control_amd.suite import common

import content_dims_models as cdm

HERE = os.path.dirname(os.path.abspath(__file__))
EFC_LIMIT = 0      # csrc/step_layout.h: EFC_TYPE(efc_tid)


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
  """tests/emu_lib.py on tests/emu/coop_open.cpp (its own copy of the module: the library is chosen at first use)."""
  spec = importlib.util.spec_from_file_location('emu_lib_coop_open', os.path.join(HERE, 'emu_lib.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  L = mod.lib(os.path.join(HERE, 'emu', 'coop_open.cpp'), 'emu_coop_open', opt='-O1', out_dir=str(tmp_path_factory.mktemp('coop_open')))
  L.emu_coop_open.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
  return mod


def _model(name):
  return cdm.alltypes() if name == 'alltypes' else mc.compile_xml(common.read_model(name + '.xml'))


def _states(mod, m, name, prec):
  """(qpos, qvel) along a rollout under random controls from a random start: in the air, on the floor, at joint limits."""
  e = mod.EmuPhysics(m, prec=prec)
  rs = np.random.RandomState(7)
  if name == 'alltypes':
    q, v = cdm.alltypes_init(m, 1, 11)
    e.qpos[:] = q[0]; e.qvel[:] = v[0]
  else:
    lim = m.jnt_limited == 1
    lo, hi = m.jnt_range[lim].T
    q = np.array(m.qpos0, dtype=np.float64)
    q[lim] = rs.uniform(lo, hi)
    e.qpos[:] = q
  e.set_mocap(np.array([[.3, .2, 1.1]] * m.nmocap), np.array([[1., 0, 0, 0]] * m.nmocap))
  out = []
  for t in range(90):
    e.ctrl[:] = rs.uniform(-1, 1, m.nu)
    e.step()
    if t % 6 == 5:
      out.append((np.array(e.qpos), np.array(e.qvel)))
  assert np.isfinite(e.qpos).all()
  return e, out


@pytest.mark.parametrize('prec', [64, 32])
@pytest.mark.parametrize('name', ['cheetah', 'hopper', 'walker', 'alltypes'])
def test_the_sides_in_either_order_leave_the_scratch_of_the_whole_stage(emu, name, prec):
  m = _model(name)
  e, states = _states(emu, m, name, prec)
  out_r = np.zeros((3, e.n_sr)); out_i = np.zeros((3, e.n_si), np.int32)
  off, cnt, kind = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
  find = lambda n: (emu.lib().emu_find(e.h, n.encode(), ctypes.byref(off), ctypes.byref(cnt), ctypes.byref(kind)), off.value, cnt.value)[1:]
  o_misc, _ = find('imisc'); o_tid, _ = find('efc_tid'); o_qm, n_qm = find('qM'); o_bias, n_bias = find('qfrc_bias')
  with_contact = with_limit = 0
  for q, v in states:
    q = np.ascontiguousarray(q, np.float64); v = np.ascontiguousarray(v, np.float64)
    assert emu.lib().emu_coop_open(e.h, prec, q.ctypes.data, v.ctypes.data, out_r.ctypes.data, out_i.ctypes.data) == 0
    # bits, not values: -0.0 and NaN payloads count
    bits = out_r.view(np.int64)
    for k, order in ((1, 'A then B'), (2, 'B then A')):
      bad = np.nonzero(bits[k] != bits[0])[0]
      assert bad.size == 0, (name, prec, order, 'real scratch differs from the whole stage at', bad[:8])
      bad = np.nonzero(out_i[k] != out_i[0])[0]
      assert bad.size == 0, (name, prec, order, 'int scratch differs from the whole stage at', bad[:8])
    ncon, nefc = int(out_i[0, o_misc + 0]), int(out_i[0, o_misc + 1])
    with_contact += ncon > 0
    with_limit += bool(((out_i[0, o_tid:o_tid + nefc] & 7) == EFC_LIMIT).any())
    # (both sides did write: a mass matrix, bias forces)
    assert np.abs(out_r[0, o_qm:o_qm + n_qm]).max() > 0 and np.abs(out_r[0, o_bias:o_bias + n_bias]).max() > 0
  assert with_contact >= 2 and with_limit >= 1, (name, prec, with_contact, with_limit)

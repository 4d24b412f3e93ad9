"""The content facts of StepDims (csrc/step_layout.h: which joint types exist, how many sensors each stage's loop has to
look at, whether any of them needs rne_post_constraint or contact forces) -- what lets a model-specialised kernel drop
the code of what its model does not contain.  No GPU.

1. What the C++ host code (step_tables_build, reached through the host build of the kernel core) computes equals the
   same facts recomputed in numpy from the compiled model's tables: every suite asset (the BASELINE models among them)
   and a hand-written model with every joint type, a mocap body, sites and one sensor of every supported type, in which
   no fact may come out empty.
2. The facts only say "may occur": the host build of the kernel core steps that model, the cheetah and the hopper to the
   same bits with the facts as computed and with -DDMC_NO_CONTENT_DIMS (everything assumed present), fp64 and fp32.
"""
import ctypes
import glob
import importlib.util
import os

import numpy as np
import pytest

from dm_control_amd import mjcf_compiler as mc
from dm_control_amd.suite import common

import content_dims_models as cdm

HERE = os.path.dirname(os.path.abspath(__file__))
ASSETS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, '..', 'dm_control_amd', 'suite', 'assets', '*.xml')))
BASELINE = ['cheetah', 'humanoid', 'cmu_2019_position_floor', 'soccer_2v2_boxhead']      # bench.py CONFIGS 2 .. 5
FIELDS = ('qpos', 'qvel', 'qacc', 'qacc_warmstart', 'sensordata', 'xpos', 'xquat', 'subtree_com', 'actuator_force', 'qfrc_constraint')


@pytest.fixture(scope='module')
def emus(tmp_path_factory):
  """tests/emu_lib.py twice, each on its own build of tests/emu/content_dims.cpp: (facts as computed, everything present)."""
  out = []
  d = str(tmp_path_factory.mktemp('content_dims'))
  for tag, flags in (('dims', []), ('nodims', ['-DDMC_NO_CONTENT_DIMS'])):
    spec = importlib.util.spec_from_file_location('emu_lib_' + tag, os.path.join(HERE, 'emu_lib.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    L = mod.lib(os.path.join(HERE, 'emu', 'content_dims.cpp'), 'emu_' + tag, flags=flags, opt='-O1', out_dir=d)
    L.emu_content_dims.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    out.append(mod)
  return out


def _facts(mod, m, **caps):
  e = mod.EmuPhysics(m, **caps)
  v = np.zeros(6, np.int32)
  built_with_dims = mod.lib().emu_content_dims(e.h, v.ctypes.data)
  return dict(zip(cdm.NAMES, (int(x) for x in v))), built_with_dims


@pytest.mark.parametrize('name', ASSETS)
def test_host_code_and_numpy_agree_on_every_suite_asset(emus, name):
  m = mc.compile_xml(common.read_model(name + '.xml'))
  caps = {k: v for k, v in common.DEFAULT_CAPS.get(name, {}).items() if k in ('nconmax', 'njmax', 'njcon')}
  got, flag = _facts(emus[0], m, **caps)
  assert flag == 1
  assert got == cdm.content_dims(m), name
  assert (got['jtypes'] != 0) == (m.njnt > 0) and got['nsens_pos'] + got['nsens_vel'] + got['nsens_acc'] <= m.nsensor


def test_the_baseline_models_are_among_the_assets():
  assert set(BASELINE) <= set(ASSETS)


def test_no_fact_drops_something_the_all_types_model_contains(emus):
  m = cdm.alltypes()
  assert m.nmocap == 1 and m.nsite == 4 and m.nv == 11 and m.nsensor == 19
  assert sorted(set(int(t) for t in m.jnt_type)) == [0, 1, 2, 3]
  got, _ = _facts(emus[0], m)
  assert got == cdm.content_dims(m)
  # by hand: 4 joint types; position stage jointpos, subtreecom, framepos, 3 frame axes, rangefinder, framequat; velocity
  # stage velocimeter, gyro, jointvel, framelinvel, frameangvel (+ the subtreelinvel sensor, which the loop skips);
  # acceleration stage touch, accelerometer, force, torque, actuatorfrc
  assert got == dict(jtypes=0b1111, nsens_pos=8, nsens_vel=5, nsens_acc=5, nsens_rne=3, nsens_touch=1)
  # the cheetah, by hand: slide and hinge joints, one subtreelinvel sensor and nothing else
  c = mc.compile_xml(common.read_model('cheetah.xml'))
  assert _facts(emus[0], c)[0] == dict(jtypes=0b1100, nsens_pos=0, nsens_vel=0, nsens_acc=0, nsens_rne=0, nsens_touch=0)
  # the reference build computes the same facts (its kernel core ignores them)
  got_ref, flag = _facts(emus[1], m)
  assert flag == 0 and got_ref == got


def _start(m, name, e):
  rs = np.random.RandomState(3)
  if name == 'alltypes':
    q, v = cdm.alltypes_init(m, 1, 11)
    e.qpos[:] = q[0]; e.qvel[:] = v[0]
    e.set_mocap(np.array([[.3, .2, 1.1]]), np.array([[.8, .2, .4, .4]]) / np.linalg.norm([.8, .2, .4, .4]))
  else:
    lim = m.jnt_limited == 1
    lo, hi = m.jnt_range[lim].T
    q = np.array(m.qpos0, dtype=np.float64)
    q[lim] = rs.uniform(lo, hi)
    e.qpos[:] = q


@pytest.mark.parametrize('prec', [64, 32])
@pytest.mark.parametrize('name', ['alltypes', 'cheetah', 'hopper'])
def test_a_step_is_the_same_bits_with_the_facts_and_with_everything_assumed_present(emus, name, prec):
  m = cdm.alltypes() if name == 'alltypes' else mc.compile_xml(common.read_model(name + '.xml'))
  pair = [mod.EmuPhysics(m, prec=prec) for mod in emus]
  for e in pair:
    _start(m, name, e)
  rs = np.random.RandomState(4)
  rows = 0
  for t in range(120):
    a = rs.uniform(-1, 1, m.nu)
    for e in pair:
      e.ctrl[:] = a
      e.step()
    rows = max(rows, int(pair[0].nefc[0]))
    for f in FIELDS:
      assert np.array_equal(getattr(pair[0], f), getattr(pair[1], f)), (name, prec, t, f)
    for f in ('ncon', 'nefc', 'solver_iter', 'warning'):
      assert np.array_equal(getattr(pair[0], f), getattr(pair[1], f)), (name, prec, t, f)
  e = pair[0]
  assert np.isfinite(e.qpos).all() and rows > 0 and np.abs(e.sensordata).max() > 0
  if name == 'alltypes':
    assert np.abs(e.qvel[cdm.FREE_DOFS]).min() > 0 and np.abs(e.qvel[cdm.BALL_DOFS]).min() > 0
    assert (np.abs(e.sensordata) > 0).sum() >= 30      # (most of the 47 sensor values: every branch of the loops wrote)

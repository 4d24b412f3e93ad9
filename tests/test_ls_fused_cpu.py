"""The fused passes of the line search's bracket phase (csrc/step_core.h primal_search, ls_eval_multi) against the
sequential search they replace: the host build of the kernel core twice, as it is and with -DDMC_NO_LS_FUSED.  No GPU.

The fused search evaluates the same points with the same arithmetic and takes the same decisions on them, only several
per pass, so the two builds must agree to the bit -- qpos, qvel, qacc_warmstart, solver_iter at every one of 300 steps under
seeded U(-1, 1) actions from the benchmark's start states, fp64 and fp32, for cheetah, hopper, walker, humanoid, the
elliptic-cone scene of tests/test_kernel_logic_emu.py and a model with an equality constraint and dof friction loss (FRICEQ
below) -- and count the same logical evaluations (emu_ls_counts()[1]).  The pass counter (emu_ls_passes, exported by
tests/emu/ls_fused.cpp) counts a fused pass once: it equals the evaluations with the switch, and is strictly smaller on
every step whose search entered the bracket phase (the entry pass alone already carries two points).

The cap: ls_iterations in {2 .. 7} puts the cap at every position inside the bracket loop.  Both builds agree to the bit
under each.  The bracket phase starts with the fourth evaluation at the earliest (p0, p1, at least one step of the
one-sided loop -- the search returns before it under a cap of 2 or 3, whatever the inputs), so that the inputs reach the
bracket phase is asserted for the caps from 4 on."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from dm_control_amd import mjcf_compiler as mc
from dm_control_amd.suite import common

import bench
from test_kernel_logic_emu import _ELLIPTIC_SCENE

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ('qpos', 'qvel', 'qacc_warmstart', 'solver_iter')
MODELS = ['cheetah', 'hopper', 'walker', 'humanoid', 'elliptic', 'friceq']
STEPS = 300
CAPS = [2, 3, 4, 5, 6, 7]
CAP_STEPS = 120

# Planar chain on the floor: dof friction loss on two hinges (Huber rows), a joint equality coupling the last two, a joint
# limit and pyramidal contacts -- the general rows of ls_eval_gen / ls_eval_ell next to one-sided ones.
FRICEQ = """
<mujoco>
  <option timestep="0.004"/>
  <worldbody>
    <geom name="floor" type="plane" size="5 5 .1"/>
    <body name="b0" pos="0 0 .3">
      <joint name="x" type="slide" axis="1 0 0"/><joint name="z" type="slide" axis="0 0 1"/><joint name="tilt" type="hinge" axis="0 1 0"/>
      <geom type="capsule" fromto="-.2 0 0 .2 0 0" size=".05" mass="2"/>
      <body name="b1" pos=".2 0 0">
        <joint name="j1" type="hinge" axis="0 1 0" range="-50 50" limited="true" damping=".1" frictionloss=".4"/>
        <geom type="capsule" fromto=".06 0 0 .4 0 0" size=".05" mass="1"/>
        <body name="b2" pos=".4 0 0">
          <joint name="j2" type="hinge" axis="0 1 0" damping=".1" frictionloss=".2"/>
          <geom type="capsule" fromto=".06 0 0 .4 0 0" size=".05" mass="1"/>
          <body name="b3" pos=".4 0 0">
            <joint name="j3" type="hinge" axis="0 1 0" damping=".1"/>
            <geom type="capsule" fromto=".06 0 0 .4 0 0" size=".05" mass="1"/>
          </body>
        </body>
      </body>
    </body>
  </worldbody>
  <equality><joint joint1="j3" joint2="j2" polycoef="0 -1 0 0 0"/></equality>
  <actuator><motor joint="j1" gear="20"/><motor joint="j2" gear="20"/></actuator>
</mujoco>
"""


@pytest.fixture(scope='module')
def emus(tmp_path_factory):
  """tests/emu_lib.py twice, each on its own build of tests/emu/ls_fused.cpp: (fused passes, the sequential search)."""
  out = []
  d = str(tmp_path_factory.mktemp('ls_fused'))
  for tag, flags in (('fused', []), ('seq', ['-DDMC_NO_LS_FUSED'])):
    spec = importlib.util.spec_from_file_location('emu_lib_ls_' + tag, os.path.join(HERE, 'emu_lib.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    L = mod.lib(os.path.join(HERE, 'emu', 'ls_fused.cpp'), 'emu_ls_' + tag, flags=flags, opt='-O1', out_dir=d)
    L.emu_ls_passes_get.argtypes = [ctypes.c_void_p]
    L.emu_set_ls_iterations.argtypes = [ctypes.c_void_p, ctypes.c_int]
    out.append(mod)
  assert _counts(out[0])[0] == 1 and _counts(out[1])[0] == 0      # which build is which
  return out


def _counts(mod):
  """(fuses, evaluations, passes, searches that entered the bracket phase, fused passes) of the build, so far."""
  c = (ctypes.c_longlong * 6)()
  p = (ctypes.c_longlong * 3)()
  mod.lib().emu_ls_counts_get(c)
  fuses = mod.lib().emu_ls_passes_get(p)
  return fuses, int(c[1]), int(p[0]), int(p[1]), int(p[2])


class _OneEnv:
  """What bench.initial_qpos asks of a batch (the humanoid's contact-free rejection test), on one emulated environment."""

  def __init__(self, e):
    self.e = e

  def set(self, name, q):
    assert name == 'qpos'
    self.e.qpos[:] = q[0]

  def forward(self, disable_actuation=False):
    self.e.forward(disable_actuation=disable_actuation)

  def get(self, name):
    assert name == 'ncon'
    return np.array([[int(self.e.ncon[0])]])


_cache = {}


def _model(name):
  if name not in _cache:
    xml = FRICEQ if name == 'friceq' else _ELLIPTIC_SCENE.format(condim=3, impratio=1.0) if name == 'elliptic' else common.read_model(name + '.xml')
    _cache[name] = mc.compile_xml(xml)
  return _cache[name]


def _start(mod, m, name):
  """The benchmark's start state of the model (cheetah, humanoid: bench.initial_qpos; hopper and walker: the cheetah's
  rule, limited joints uniform in their range), the elliptic scene with the velocities of its own test, the chain dropped."""
  caps = {k: v for k, v in common.DEFAULT_CAPS.get(name, {}).items() if k in ('nconmax', 'njmax', 'njcon')}
  q = v = None
  if name in ('cheetah', 'hopper', 'walker'):
    q = bench.initial_qpos(dict(asset='cheetah'), m, 1, 0)[0]
  elif name == 'humanoid':
    q = bench.initial_qpos(dict(asset='humanoid'), m, 1, 0, phys=_OneEnv(mod.EmuPhysics(m, 64, **caps)))[0]
  elif name == 'elliptic':
    v = np.random.RandomState(3).uniform(-1, 1, m.nv)
  else:
    q = np.array(m.qpos0, dtype=np.float64)
    q[3:] += np.random.RandomState(1).uniform(-.5, .5, m.nq - 3)
  return caps, q, v


def _run(emus, name, prec, steps, cap=None):
  """Steps the model on both builds; bit-equality at every step.  Returns per step (evaluations, passes, bracket entries) of
  the fused build and the totals of the sequential one."""
  m = _model(name)
  pair = []
  for mod in emus:
    caps, q, v = _start(mod, m, name)
    e = mod.EmuPhysics(m, prec, **caps)
    if q is not None:
      e.qpos[:] = q
    if v is not None:
      e.qvel[:] = v
    if cap is not None:
      mod.lib().emu_set_ls_iterations(e.h, cap)
    pair.append(e)
  rs = np.random.RandomState(1234)
  per_step = []
  tot = [np.zeros(5, np.int64), np.zeros(5, np.int64)]
  for t in range(steps):
    a = rs.uniform(-1, 1, m.nu)
    for k, (mod, e) in enumerate(zip(emus, pair)):
      # (the counters are function-local statics of an inline function: the loader may give both builds ONE object, so
      # each build's share is what its own step adds)
      before = np.array(_counts(mod))
      e.ctrl[:] = a
      e.step()
      d = np.array(_counts(mod)) - before
      tot[k] += d
      if k == 0:
        per_step.append((int(d[1]), int(d[2]), int(d[3])))
    for f in FIELDS:
      assert np.array_equal(getattr(pair[0], f), getattr(pair[1], f)), (name, prec, cap, t, f)
  assert np.isfinite(pair[0].qpos).all()
  return per_step, [tuple(int(x) for x in v) for v in tot]


@pytest.mark.parametrize('prec', [64, 32])
@pytest.mark.parametrize('name', MODELS)
def test_fused_and_sequential_search_agree_to_the_bit(emus, name, prec):
  per_step, (fused, seq) = _run(emus, name, prec, STEPS)
  print('measured: %s fp%d over %d steps: evaluations %d (sequential build %d), passes %d (sequential build %d), searches '
        'in the bracket phase %d, fused passes %d' % (name, prec, STEPS, fused[1], seq[1], fused[2], seq[2], fused[3], fused[4]))
  assert fused[1] == seq[1] and fused[1] > 0      # the same logical evaluations
  assert seq[2] == seq[1] and seq[4] == 0          # the switch: a pass per evaluation
  assert fused[3] == seq[3]                        # the same searches entered the bracket phase
  for t, (ev, ps, br) in enumerate(per_step):
    if br:
      assert ps < ev, (name, prec, t, ev, ps, br)
    else:
      assert ps == ev, (name, prec, t, ev, ps)
  assert fused[3] > 0, 'no search of %s fp%d entered the bracket phase' % (name, prec)


@pytest.mark.parametrize('cap', CAPS)
def test_the_cap_on_evaluations_keeps_its_meaning(emus, cap):
  entered = 0
  for name in MODELS:
    for prec in (64, 32):
      _, (fused, seq) = _run(emus, name, prec, CAP_STEPS, cap=cap)
      assert fused[1] == seq[1] and fused[3] == seq[3], (name, prec, cap, fused, seq)
      entered += fused[3]
  print('measured: ls_iterations = %d: searches that entered the bracket phase %d' % (cap, entered))
  if cap >= 4:      # (the fourth evaluation is the first the bracket phase can make: module docstring)
    assert entered > 0
  else:
    assert entered == 0

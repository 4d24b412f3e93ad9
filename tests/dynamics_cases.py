"""TEST INFRASTRUCTURE: the shared cases of the dynamics unit's tests (tests/test_dynamics_cpu.py, tests/test_gpu_dynamics.py).

The fixture is the model of tests/jacobian_cases.py -- a free body, a ball joint, a slide and a hinge on one body, a
three-hinge arm, free boxes -- with gravity, armature and damping switched on, at eight boxes (nv = 62, 15 bodies: a batch
holds nv <= 64); its states are jacobian_cases.states (16 states, seed 2024).  Beside it: the suite's cheetah (nv = 9,
16 lanes per environment), humanoid (nv = 27), the CMU humanoid (a deep sparse tree), a small model with a mocap body
beside the jointed tree, and the fixture with gravity disabled.

References, none of them the code under test: the fp64 oracle after forward() -- qM (dense), qfrc_bias, qfrc_smooth,
qacc_smooth -- and host_data.mass_matrix; numpy.linalg.solve for the solves.
"""
import numpy as np

import jacobian_cases as jc
from dm_control_amd import host_data

NBOX = 8
NSTATE = jc.NSTATE
SEED = jc.SEED
F64_TOL = 1e-9      # x max(1, |reference|max): the project's bar for its fp64 units
# fp32: the worst error of the fp32 HOST build of csrc/dyn_core.h against the references over every model and state of the
# CPU tier (measured and printed by test_dynamics_cpu.py::test_host_build_meets_the_bounds_on_every_model), relative to
# max(1, |reference|max); for `solve` the elementwise backward error |qM x - f| / (|qM| |x| + |f|) -- the forward error
# scales with cond(M), a property of the model.  The bound is 4 x the measured value, on the CPU and on the GPU.
# `inverse_smooth` is inverse() at the oracle's qacc_smooth against qfrc_smooth + qfrc_bias: those accelerations reach 1e3 and
# M qacc cancels against the bias, so it has a bound of its own and the random-qacc cases keep their tighter one.
F32_MEASURED = dict(M=2.27e-7, bias=1.04e-6, inverse=3.66e-7, inverse_smooth=4.10e-5, mul=4.57e-7, solve=7.47e-6)
F32_TOL = {k: 4 * v for k, v in F32_MEASURED.items()}
OUTPUTS = ('M', 'bias', 'inverse', 'mul', 'solve')
K = 3               # right-hand sides per environment in the shared cases
# The fixture's states with a contact (state: ncon): a box touches the arm.  qM, qfrc_bias, qacc_smooth and qfrc_smooth are
# computed before the constraint solve and do not see it, so these states stay in; every other state has ncon == 0.
CONTACT_STATES = {6: 1, 12: 2}

MOCAP_XML = """<mujoco model="mocap_beside_tree">
  <option gravity="0 0 -9.81"/>
  <worldbody>
    <body name="target" mocap="true" pos=".4 .1 .9"><geom name="tg" type="sphere" size=".05" mass="3"/>
      <body name="welded" pos="0 0 .2"><geom type="box" size=".03 .03 .03" mass="2"/></body>
    </body>
    <body name="base" pos="0 0 .5" quat=".9 .1 .2 .1">
      <geom type="box" size=".1 .1 .05" mass="5"/>
      <body name="arm" pos=".1 0 .1">
        <joint name="sh" type="hinge" axis="0 1 .2" pos="0 .01 0" armature=".02"/>
        <geom type="capsule" size=".03 .15" pos=".15 0 0" quat=".7 0 .7 0" mass="1.5"/>
        <body name="fore" pos=".3 0 0" quat=".95 0 .2 .1">
          <joint name="el" type="hinge" axis="1 0 0"/>
          <joint name="ex" type="slide" axis="0 .3 1" ref=".05"/>
          <geom type="capsule" size=".02 .1" pos="0 0 -.1" mass=".8"/>
        </body>
      </body>
    </body>
    <body name="puck" pos="1 0 .2"><joint name="pj" type="free"/><geom type="cylinder" size=".08 .02" mass=".4"/></body>
  </worldbody>
</mujoco>"""


def xml(nbox=NBOX, gravity=True):
  x = jc.xml(nbox)
  assert '<option gravity="0 0 0"/>' in x
  opt = '<option gravity="0 0 -9.81"/>' if gravity else '<option gravity="0 0 -9.81"><flag gravity="disable"/></option>'
  return x.replace('<option gravity="0 0 0"/>', opt + '\n  <default><joint armature="0.01" damping="0.1"/></default>')


def model_xml(name):
  from dm_control_amd.suite import common      # pylint: disable=import-outside-toplevel
  if name == 'fixture':
    return xml()
  if name == 'fixture_nogravity':
    return xml(gravity=False)
  if name == 'mocap':
    return MOCAP_XML
  return common.read_model(name + '.xml')


MODELS = ('fixture', 'cheetah', 'humanoid', 'humanoid_CMU', 'mocap', 'fixture_nogravity')
_models = {}


def model(name='fixture'):
  if name not in _models:
    from dm_control_amd import mjcf_compiler      # pylint: disable=import-outside-toplevel
    _models[name] = mjcf_compiler.compile_xml(model_xml(name))
  return _models[name]


def states(m, n=NSTATE, seed=SEED):
  return jc.states(m, n, seed)


def inputs(nv, n=NSTATE, k=K, seed=SEED + 1):
  """(qacc (n, nv), vec (n, k, nv)) in [-1, 1]: the accelerations of inverse() and the vectors of mul() / solve()."""
  rs = np.random.RandomState(seed)
  return rs.uniform(-1, 1, (n, nv)), rs.uniform(-1, 1, (n, k, nv))


def dense(qM, nv):
  qM = np.asarray(qM, dtype=np.float64)
  assert qM.size == nv * nv, 'the oracle holds qM dense (nv x nv)'
  return qM.reshape(nv, nv).copy()


def reference(m, qpos, qvel, qacc, vec):
  """The references of one state from the fp64 oracle after forward(): dict(M, M_host (host_data.mass_matrix), bias,
  inverse (qM qacc + qfrc_bias), mul (qM vec'), solve (numpy.linalg.solve), qacc_smooth, inverse_smooth (qfrc_smooth +
  qfrc_bias), ncon)."""
  from oracle.oracle import OraclePhysics      # pylint: disable=import-outside-toplevel
  p = OraclePhysics(m)
  p.qpos[:] = qpos
  p.qvel[:] = qvel
  p.forward()
  nv = m.nv
  M = dense(p.qM, nv)
  g = lambda n, *s: np.array(p.field(n), dtype=np.float64).reshape(*s)
  xpos, xquat = g('xpos', -1, 3), g('xquat', -1, 4)
  anchor, axis = host_data.joint_frames(m, np.asarray(qpos, dtype=np.float64), xpos, xquat)
  Mh = host_data.mass_matrix(m, xpos, g('xmat', -1, 9), g('xipos', -1, 3), g('ximat', -1, 9), anchor, axis)
  bias = g('qfrc_bias', nv)
  vec = np.asarray(vec, dtype=np.float64).reshape(-1, nv)
  return dict(M=M, M_host=Mh, bias=bias, inverse=M @ qacc + bias, mul=vec @ M.T, solve=np.linalg.solve(M, vec.T).T,
              qacc_smooth=g('qacc_smooth', nv), inverse_smooth=g('qfrc_smooth', nv) + bias, ncon=int(p.ncon),
              xpos=xpos, xquat=xquat)


def backward_error(M, x, f):
  """Elementwise backward error of a solve: max |M x - f| / (|M| |x| + |f|)."""
  M, x, f = (np.asarray(a, dtype=np.float64) for a in (M, x, f))
  x, f = x.reshape(-1, M.shape[0]), f.reshape(-1, M.shape[0])
  num = np.abs(x @ M.T - f)
  den = np.abs(x) @ np.abs(M).T + np.abs(f)
  return float(np.max(num / np.maximum(den, np.finfo(np.float64).tiny)))


def errors(got, ref, vec):
  """{output: error relative to max(1, |reference|max)} of the outputs in `got`; solve: the backward error against the
  reference M, and `solve_forward`: |x - x_ref| relative likewise."""
  out = {}
  for k, v in got.items():
    r = ref[k]
    out[k] = float(np.abs(np.asarray(v) - r).max() / max(1.0, np.abs(r).max()))
    if k == 'solve':
      out['solve_forward'] = out[k]
      out[k] = backward_error(ref['M'], v, vec)
  return out


def bound(prec, key):
  """fp64: 1e-9 (x max(1, |reference|max), also for the forward error of solve); fp32: F32_TOL[key]."""
  return F64_TOL if prec == 64 else F32_TOL[key]


def check(got, ref, vec, prec, where=()):
  """Asserts the bounds on every output of `got`; returns the errors.  fp64 solve is judged forward (1e-9 is reachable:
  cond(M) <= 1.2e3 for the fixture); fp32 solve backward."""
  err = errors(got, ref, vec)
  for k in got:
    e = err['solve_forward'] if (k == 'solve' and prec == 64) else err[k]
    assert e <= bound(prec, k), (where, k, prec, e)
  return err

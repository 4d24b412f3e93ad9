"""TEST INFRASTRUCTURE: the shared cases of the linearisation unit's tests (tests/test_linearize_cpu.py,
tests/test_gpu_linearize.py).

Models, small on purpose: `leg` (nq 13, nv 11, na 1, nu 3, 8 sensor values: a free trunk over a floor, a ball hip, a limited
hinge knee, a limited slide with a sphere foot; a ctrllimited motor and a filter-dynamics general on the knee, a ctrllimited
position servo on the slide; accelerometer, gyro, jointpos, actuatorfrc), the suite's cheetah (nv 9, nu 6, P = 49), humanoid
(nv 27, a free root, nu 21, P = 151), lqr_2_1 (slide joints: a linear system) and acrobot (RK4).

States: reset, then a seeded number of steps under small random controls, so that contact-free and in-contact states both
occur; the linearisation point's control is a further small random draw.  NCON records the contacts of each state.

The reference is tests/lin_twin.py (a numpy mjd_transitionFD on the fp64 oracle), for lqr_2_1 also a closed form.
"""
import numpy as np

SEED = 2025
EPS = 1e-6
EPS32 = 2.0 ** -10      # the nudge of the fp32-scratch mode
F64_TOL = 1e-9          # x max(1, |reference|max): the project's bar for its fp64 units

LEG_XML = """<mujoco model="leg">
  <option timestep="0.002"/>
  <worldbody>
    <geom name="floor" type="plane" size="5 5 .1"/>
    <body name="trunk" pos="0 0 .9">
      <joint name="root" type="free"/>
      <geom name="trunk" type="box" size=".12 .08 .06" mass="4"/>
      <site name="imu" pos="0 0 .02"/>
      <body name="thigh" pos="0 0 -.08">
        <joint name="hip" type="ball" damping=".2"/>
        <geom name="thigh" type="capsule" fromto="0 0 0 0 0 -.3" size=".04" mass="1.5"/>
        <body name="shin" pos="0 0 -.3">
          <joint name="knee" type="hinge" axis="0 1 0" limited="true" range="-2 .1" damping=".1"/>
          <geom name="shin" type="capsule" fromto="0 0 0 0 0 -.25" size=".03" mass=".8"/>
          <body name="foot" pos="0 0 -.25">
            <joint name="ankle" type="slide" axis="0 0 1" limited="true" range="-.08 .08" stiffness="300" damping="3"/>
            <geom name="foot" type="sphere" size=".05" pos="0 0 -.08" mass=".3"/>
          </body>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator>
    <motor name="knee_m" joint="knee" gear="30" ctrllimited="true" ctrlrange="-1 1"/>
    <general name="knee_f" joint="knee" gear="10" dyntype="filter" dynprm=".05" gainprm="1"/>
    <position name="ankle_p" joint="ankle" kp="200" ctrllimited="true" ctrlrange="-.05 .05"/>
  </actuator>
  <sensor>
    <accelerometer name="acc" site="imu"/>
    <gyro name="gyro" site="imu"/>
    <jointpos name="knee_q" joint="knee"/>
    <actuatorfrc name="knee_f" actuator="knee_m"/>
  </sensor>
</mujoco>"""

MODELS = ('leg', 'cheetah', 'humanoid', 'lqr_2_1', 'acrobot')
# steps taken from the reset pose before the linearisation point, per model: one state each
STEPS = dict(leg=(50, 150, 1200, 1100), cheetah=(0, 100, 240), humanoid=(10, 160), lqr_2_1=(5, 60), acrobot=(25, 140))
# contacts of those states (the fp64 oracle; checked by test_linearize_cpu.py::test_states_are_as_recorded)
NCON = dict(leg=(0, 1, 2, 4), cheetah=(0, 2, 1), humanoid=(0, 5), lqr_2_1=(0, 0), acrobot=(0, 0))
LIMIT_CTRL = (1.0, 0.3, -0.05)      # leg: the motor at its upper limit, the servo at its lower one
# environments of the batches the GPU tier shares, which the fp32 measurement of the CPU tier walks too: (state index,
# control or None: the state's own)
ENVS = dict(leg=[(0, None), (1, None), (2, None), (3, None), (1, LIMIT_CTRL)], cheetah=[(0, None), (1, None), (2, None)],
            humanoid=[(0, None), (1, None)], acrobot=[(0, None), (1, None)])
_models, _states = {}, {}


def model_xml(name):
  from dm_control_amd.suite import common      # pylint: disable=import-outside-toplevel
  if name == 'leg':
    return LEG_XML
  if name == 'lqr_2_1':
    from dm_control_amd.suite import lqr      # pylint: disable=import-outside-toplevel
    return lqr.get_model_and_assets(2, 1, np.random.RandomState(SEED))[0]
  return common.read_model(name + '.xml')


def model(name='leg'):
  if name not in _models:
    from dm_control_amd import mjcf_compiler      # pylint: disable=import-outside-toplevel
    _models[name] = mjcf_compiler.compile_xml(model_xml(name))
  return _models[name]


def states(name):
  """[dict(qpos, qvel, act, ctrl, qacc_warmstart, qfrc_applied, time, ncon)] of model `name`, one per entry of STEPS."""
  if name not in _states:
    from oracle.oracle import OracleModel, OraclePhysics      # pylint: disable=import-outside-toplevel
    m = model(name)
    om = OracleModel(m)
    out = []
    for n in STEPS[name]:
      rs = np.random.RandomState(SEED + n)
      p = OraclePhysics(om, legacy_step=False)
      if name in ('lqr_2_1', 'acrobot'):      # (their reset poses are equilibria: start away from them)
        p.qpos[:] = p.qpos + rs.uniform(-.3, .3, m.nq)
      p.forward()
      for _ in range(n):
        if m.nu:
          p.ctrl[:] = rs.uniform(-.3, .3, m.nu) * ctrl_scale(m)
        p.step(1)
      g = lambda f, rows: np.array(p.field(f), dtype=np.float64).ravel().copy() if rows else np.zeros(0)
      s = dict(qpos=g('qpos', m.nq), qvel=g('qvel', m.nv), act=g('act', m.na), qacc_warmstart=g('qacc_warmstart', m.nv),
               ctrl=rs.uniform(-.3, .3, m.nu) * ctrl_scale(m), qfrc_applied=np.zeros(m.nv), time=np.array([p.time]))
      p2 = OraclePhysics(om, legacy_step=False)      # the contacts AT the state
      p2.qpos[:] = s['qpos']
      p2.forward()
      s['ncon'] = int(p2.ncon)
      out.append(s)
    _states[name] = out
  return _states[name]


def env_states(name, envs=None):
  """The states of ENVS[name] (or of `envs`), each with its control put in."""
  envs = ENVS[name] if envs is None else envs
  return [dict(states(name)[i], **({} if c is None else dict(ctrl=np.array(c, dtype=np.float64)))) for i, c in envs]


def ctrl_scale(m):
  """Per actuator: half the width of ctrlrange where limited (so that +-0.3 of it stays inside), else 1."""
  cr = np.asarray(m.actuator_ctrlrange, dtype=np.float64).reshape(-1, 2)
  lim = np.asarray(m.actuator_ctrllimited).astype(bool)
  return np.where(lim, 0.5 * (cr[:, 1] - cr[:, 0]), 1.0)


def rel_err(got, ref):
  """|got - ref|max relative to max(1, |ref|max)."""
  got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
  if not ref.size:
    return 0.0
  return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def worst(got, ref):
  """The worst rel_err over A, B, C, D (`got`, `ref`: sequences or dicts of the four)."""
  if isinstance(ref, dict):
    ref = [ref[k] for k in 'ABCD']
  if isinstance(got, dict):
    got = [got[k] for k in 'ABCD']
  return max(rel_err(g, r) for g, r in zip(got, ref))


# ---- measured errors and the bounds made of them ---------------------------------------------------------------------
# Worst error of the fp64 host pipeline (host fan-out, the oracle's mj_step per column, host difference) against the twin at
# equal eps, relative to max(1, |ref|max), per model over its states; printed by test_linearize_cpu.py::test_pipeline.
# Contact-free states have to meet F64_TOL; for the states in contact the bound is 4 x the measured worst.
PIPELINE_F64_MEASURED = dict(leg=6.5e-17, cheetah=0.0, humanoid=1.3e-16, lqr_2_1=0.0, acrobot=0.0)
# The fp32 host pipeline (fan-out and difference in fp32, the columns stepped by the fp32 host build of the step core,
# tests/emu_lib.py) against the fp64 twin at the same fp32 state, both at EPS32: what precision=32 gives.  Bound = 4 x
# measured, on the CPU and for the device's fp32-scratch mode.
PIPELINE_F32_MEASURED = dict(leg=9.83e-4, cheetah=1.18e-4)      # (leg: the one-sided column of the clamped motor; 1.70e-4 without it)
# The device's fp64 scratch batch end to end against the twin evaluated on the state the device holds: key -> (worst over
# the contact-free environments, worst over the environments in contact) of the batches of tests/test_gpu_linearize.py,
# which prints them.  The device's step agrees with the oracle's to about 1e-14 of the next state, not to the bit, and a
# quotient at eps = 1e-6 magnifies that a million times.  Contact-free environments keep the CPU tier's F64_TOL where the
# measurement meets it; everywhere else the CPU tier's bound is out of reach by construction and the bound is 4 x the
# measurement.
DEVICE_MEASURED = dict(leg=(2.27e-10, 9.94e-10), cheetah=(1.75e-10, 5.96e-10), humanoid=(9.65e-9, 5.36e-10),
                       leg_nstep3=(2.05e-10, 2.00e-9), leg_forward=(3.57e-10, 1.56e-9), acrobot=(0.0, 0.0),
                       leg_limits=(0.0, 2.08e-9), leg_limits_forward=(0.0, 3.72e-9))      # (the limits batches hold no contact-free state)
# The fp32-scratch mode on the device against the fp64 twin at EPS32 (bound: 4 x PIPELINE_F32_MEASURED): leg 1.23e-3, cheetah 1.27e-4.


def device_bound(key, kind):
  """The bound of a device result against the twin for `kind` ('free' / 'contact') environments."""
  free, contact = DEVICE_MEASURED[key]
  if kind == 'free':
    return F64_TOL if free <= F64_TOL else 4 * free
  return 4 * contact

"""TEST INFRASTRUCTURE: the model of tests/test_content_dims_cpu.py and tests/test_gpu_fixed_stages.py that contains
everything the content facts of StepDims (csrc/step_layout.h) speak about, and those facts recomputed in numpy.

ALLTYPES: a free joint, a ball joint, a body with two joints (slide + hinge, both limited), a mocap body, sites, two
actuators and one sensor of every supported type.  11 dofs; only the three spheres touch the floor (pyramidal contacts of
four rows each), so with the two joint limits an environment never has more than 14 constraint rows: a model-specialised
fp32 kernel keeps every solve of it in registers."""
import numpy as np

from dm_control_amd import mjcf_compiler as mc

ALLTYPES = """
<mujoco>
  <option timestep="0.004"/>
  <worldbody>
    <geom name="floor" type="plane" size="5 5 .1" contype="0" conaffinity="1"/>
    <body name="target" mocap="true" pos=".4 .3 1.2" quat="1 0 0 0">
      <geom type="sphere" size=".03" contype="0" conaffinity="0"/>
      <site name="goal"/>
    </body>
    <body name="base" pos="0 0 .6">
      <freejoint name="root"/>
      <geom name="g_base" type="sphere" size=".12" mass="2" contype="1" conaffinity="0"/>
      <site name="imu" pos=".02 .01 .03" quat=".9 .1 .2 .3"/>
      <body name="arm" pos=".3 0 0">
        <joint name="ball" type="ball" pos="-.15 0 0" damping=".05"/>
        <geom name="g_arm" type="sphere" size=".1" mass="1" contype="1" conaffinity="0"/>
        <site name="tip" pos=".05 0 0" quat=".8 .2 .1 .5"/>
        <body name="hand" pos=".3 0 0">
          <joint name="slide" type="slide" axis="1 0 0" range="-.1 .1" limited="true" damping=".5"/>
          <joint name="hinge" type="hinge" axis="0 1 0" pos="-.1 0 0" range="-60 60" limited="true" damping=".05"/>
          <geom name="g_hand" type="sphere" size=".08" mass=".5" contype="1" conaffinity="0"/>
          <site name="pad" type="sphere" size=".12"/>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator><motor name="a_slide" joint="slide" gear="5"/><motor name="a_hinge" joint="hinge" gear="2"/></actuator>
  <sensor>
    <touch site="pad"/><accelerometer site="imu"/><velocimeter site="imu"/><gyro site="tip"/><force site="tip"/><torque site="tip"/>
    <jointpos joint="hinge"/><jointvel joint="slide"/><actuatorfrc actuator="a_hinge"/>
    <subtreecom body="base"/><subtreelinvel body="arm"/>
    <framepos objtype="site" objname="tip"/><framexaxis objtype="body" objname="arm"/><frameyaxis objtype="xbody" objname="hand"/>
    <framezaxis objtype="geom" objname="g_hand"/><rangefinder site="imu"/><framequat objtype="site" objname="goal"/>
    <framelinvel objtype="site" objname="pad"/><frameangvel objtype="body" objname="hand"/>
  </sensor>
</mujoco>
"""
FREE_DOFS, BALL_DOFS = slice(0, 6), slice(6, 9)
NAMES = ('jtypes', 'nsens_pos', 'nsens_vel', 'nsens_acc', 'nsens_rne', 'nsens_touch')      # StepDims, in its order


def alltypes():
  return mc.compile_xml(ALLTYPES)


def alltypes_init(m, B, seed):
  """Start states in the air and on the floor, tumbling: every joint type moves."""
  rs = np.random.RandomState(seed)
  q = np.tile(m.qpos0, (B, 1))
  q[:, 2] = rs.uniform(0.15, 0.9, B)
  quat = rs.randn(B, 4)
  q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
  quat = rs.randn(B, 4)
  q[:, 7:11] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
  q[:, 11] = rs.uniform(-.08, .08, B)
  q[:, 12] = rs.uniform(-.9, .9, B)
  v = rs.uniform(-1, 1, (B, m.nv))
  return q, v


def content_dims(m):
  """The content facts from the compiled model's integer tables."""
  C = mc.C
  ty = np.asarray(m.sensor_type).astype(int)
  st = np.asarray(m.sensor_needstage).astype(int)
  loop = ty != C['DMC_SENS_SUBTREELINVEL']
  acc = st == C['DMC_STAGE_ACC']
  jt = 0
  for t in np.asarray(m.jnt_type).astype(int):
    jt |= 1 << int(t)
  return dict(jtypes=jt,
              nsens_pos=int((loop & (st == C['DMC_STAGE_POS'])).sum()), nsens_vel=int((loop & (st == C['DMC_STAGE_VEL'])).sum()),
              nsens_acc=int(acc.sum()),
              nsens_rne=int((acc & np.isin(ty, [C['DMC_SENS_ACCELEROMETER'], C['DMC_SENS_FORCE'], C['DMC_SENS_TORQUE']])).sum()),
              nsens_touch=int((acc & (ty == C['DMC_SENS_TOUCH'])).sum()))

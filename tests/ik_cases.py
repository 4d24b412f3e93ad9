"""TEST INFRASTRUCTURE: the models, targets and start states the inverse-kinematics tests share."""
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(_HERE, 'golden', 'ik_arm_reference.json')

SITE = 'gripsite'
ARM_JOINTS = ['joint_1', 'joint_2', 'joint_3', 'joint_4', 'joint_5', 'joint_6']
# the 14 targets of the reference's inverse_kinematics_test.py (data: positions and unnormalised quaternions)
ARM_TARGETS = [
    ((0., 0., 0.3), (0., 1., 0., 1.)), ((-0.5, 0., 0.5), None), ((0., 0., 0.8), (0., 1., 0., 1.)), ((0., 0., 0.8), None),
    ((0., -0.1, 0.5), None), ((0., -0.1, 0.5), (1., 1., 0., 0.)), ((0.5, 0., 0.5), None), ((0.4, 0.1, 0.5), None),
    ((0.4, 0.1, 0.5), (1., 0., 0., 0.)), ((0., 0., 0.3), None), ((0., 0.5, -0.2), None), ((0.5, 0., 0.3), (1., 0., 0., 1.)),
    (None, (1., 0., 0., 1.)), (None, (0., 1., 0., 1.)),
]
REF_TOL = 1.2e-14      # the tolerance the reference's test asks for
MAX_RESETS = 10
# fp32: |err_norm evaluated in fp32 - err_norm evaluated in fp64| at the same fp32 qpos, the largest over the arm's 14
# targets at the point where the fp32 iteration stalls (2.24e-7), times the margin of 4 DESIGN.md section 8 gives an
# fp32 bound set from one measurement
KIN_ROUNDING_F32 = 4 * 2.24e-7

# Tolerance of the step-for-step comparisons on randomly drawn targets (the inline chain): an fp64 error norm of a chain
# about a metre long carries ~1e-15 of absolute rounding, so `err_norm < 1e-14` is decided by that rounding whenever the
# quadratically converging error lands within ~10 % of the tolerance (seen: 9.98e-15).  1e-12 is a thousand times the
# rounding; the arm's fixed cases keep the reference's own tolerance.
CHAIN_TOL = 1e-12

# a free, a slide, a hinge and a ball joint between the world and the site
CHAIN_XML = """
<mujoco>
  <worldbody>
    <body name="base" pos="0 0 0.5">
      <freejoint name="root"/>
      <geom type="sphere" size="0.05"/>
      <body name="b1" pos="0.1 0 0">
        <joint name="s" type="slide" axis="1 0.5 0"/>
        <geom type="sphere" size="0.03"/>
        <body name="b2" pos="0 0.1 0" quat="0.9 0.1 0.2 0.3">
          <joint name="h" type="hinge" axis="0 1 1" pos="0.02 0 0.01"/>
          <geom type="sphere" size="0.03"/>
          <body name="b3" pos="0 0 0.15">
            <joint name="ball" type="ball" pos="0 0.01 0"/>
            <geom type="sphere" size="0.03"/>
            <site name="tip" pos="0.05 0.02 0.1" quat="0.7 0.1 0.5 0.2"/>
          </body>
        </body>
      </body>
    </body>
    <body name="other" pos="1 1 1">
      <joint name="aside" type="hinge" axis="0 0 1"/>
      <geom type="sphere" size="0.03"/>
    </body>
  </worldbody>
</mujoco>
"""


def xml(name):
  with open(os.path.join(_HERE, 'golden', 'mujoco_testing_%s.xml' % name)) as f:
    return f.read()


def model(name):
  from dm_control_amd import mjcf_compiler
  return mjcf_compiler.compile_xml(CHAIN_XML if name == 'chain' else xml(name))


def arm_start(model_, target, seed):
  """Start state `seed` of target `target`: joints 1-6 uniform over their range, or over [0, 2 pi) where unlimited (as
  the reference's test resets the arm)."""
  rs = np.random.RandomState(100 * target + seed)
  q = np.array(model_.qpos0, dtype=np.float64)
  for k, name in enumerate(ARM_JOINTS):
    j = model_.names['joint'].index(name)
    lo, hi = (model_.jnt_range[j] if model_.jnt_limited[j] else (0.0, 2 * np.pi))
    q[int(model_.jnt_qposadr[j])] = rs.uniform(lo, hi)
  return q


def arm_cases(model_):
  """The 42 (target index, seed, target_pos, target_quat, start qpos) cases of the golden file."""
  out = []
  for t, (tp, tq) in enumerate(ARM_TARGETS):
    for seed in range(3):
      out.append((t, seed, None if tp is None else np.array(tp), None if tq is None else np.array(tq), arm_start(model_, t, seed)))
  return out


def random_qpos(model_, rs, scale=1.0):
  """A random configuration: hinges / slides uniform in [-scale, scale], unit quaternions for ball / free rotations."""
  q = np.array(model_.qpos0, dtype=np.float64)
  for j in range(model_.njnt):
    t, a = int(model_.jnt_type[j]), int(model_.jnt_qposadr[j])
    if t == 0:
      q[a:a + 3] += rs.uniform(-scale, scale, 3)
      v = rs.normal(size=4)
      q[a + 3:a + 7] = v / np.linalg.norm(v)
    elif t == 1:
      v = rs.normal(size=4)
      q[a:a + 4] = v / np.linalg.norm(v)
    else:
      q[a] += rs.uniform(-scale, scale)
  return q


def golden():
  with open(GOLDEN) as f:
    return json.load(f)


def long_chain_xml(n=20):
  """`n` ball joints in a row, 0.1 m apart, the site `end` at the tip: so many chain dofs that a wave seats fewer than 64
  environments."""
  links = ''.join('<body pos="0.02 0 0.1"><joint name="k%d" type="ball"/><geom type="sphere" size="0.01"/>' % k for k in range(n))
  return '<mujoco><worldbody>%s<site name="end" pos="0 0.01 0.05"/>%s</worldbody></mujoco>' % (links, '</body>' * n)

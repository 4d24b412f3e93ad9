"""TEST INFRASTRUCTURE: the small model of tests/test_data_fields_cpu.py and tests/test_gpu_fields.py -- every data field
of include/dmc_model_layout.h has rows in it: a mocap body (nmocap = 1), an actuator with an activation state (na = 1),
a site, a sensor, and one contact pair (a box on the floor: up to four contacts, the cap; the mocap geom collides
with nothing)."""
from dm_control_amd import mjcf_compiler as mc

NCONMAX = 4
XML = """
<mujoco>
  <option timestep="0.002"/>
  <worldbody>
    <geom name="floor" type="plane" size="2 2 .1"/>
    <body name="target" mocap="true" pos=".5 0 .5"><geom name="t" size=".05" contype="0" conaffinity="0"/></body>
    <body name="box" pos="0 0 .1">
      <joint name="z" type="slide" axis="0 0 1"/><joint name="y" type="hinge" axis="0 1 0"/>
      <geom name="g" type="box" size=".1 .1 .1"/><site name="s" pos=".1 0 0"/>
    </body>
  </worldbody>
  <actuator><general name="a" joint="y" dyntype="integrator" gainprm="2"/><motor name="m" joint="z"/></actuator>
  <sensor><jointpos joint="y"/></sensor>
</mujoco>
"""


def model():
  return mc.compile_xml(XML)

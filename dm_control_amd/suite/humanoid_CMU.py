"""Humanoid_CMU domain (reference: dm_control/suite/humanoid_CMU.py): stand, walk, run.

62 degrees of freedom, 56 motors, capsule limbs, sphere toes and two ellipsoid hands that collide with
the whole body (1118 candidate pairs): the ellipsoid pairs use the iterative support-function narrow
phase (csrc/step_geom.h `ellipsoid_pair`).  The task is the suite humanoid's with the thorax as torso
(uprightness = thorax y axis on world z) and `l` / `r` limb prefixes, so it is built from that
module's classes."""
from dm_control_amd.envs import control
from dm_control_amd.suite import common
from dm_control_amd.suite import humanoid

_DEFAULT_TIME_LIMIT = 20
_CONTROL_TIMESTEP = 0.02
_WALK_SPEED = 1
_RUN_SPEED = 10
TASKS = {}


def get_model_and_assets():
  return common.read_model('humanoid_CMU.xml'), None


class Physics(humanoid.Physics):
  TORSO = 'thorax'
  UPRIGHT_AXIS = 'zy'
  SIDES = ('l', 'r')
  COM_VELOCITY_SENSOR = 'thorax_subtreelinvel'

  def thorax_upright(self):
    """Projection of the thorax y axis on the world z axis (humanoid_CMU.py:84-86)."""
    return self.torso_upright()


class HumanoidCMU(humanoid.Humanoid):
  """Stand / walk / run with egocentric features (humanoid_CMU.py:113-190): initial pose by rejection
  sampling, observations and reward exactly as the humanoid's (same stand height, 1.4 m)."""

  def __init__(self, move_speed, random=None):
    super().__init__(move_speed=move_speed, pure_state=False, random=random)


def _make(move_speed):
  def factory(time_limit=_DEFAULT_TIME_LIMIT, random=None, environment_kwargs=None, physics_kwargs=None):
    physics = Physics.from_xml_string(*get_model_and_assets(), **common.physics_kwargs('humanoid_CMU', physics_kwargs))
    return control.Environment(physics, HumanoidCMU(move_speed=move_speed, random=random), time_limit=time_limit,
                               control_timestep=_CONTROL_TIMESTEP, **(environment_kwargs or {}))
  return factory


stand, walk, run = _make(0), _make(_WALK_SPEED), _make(_RUN_SPEED)
TASKS.update(stand=(stand, None), walk=(walk, None), run=(run, None))

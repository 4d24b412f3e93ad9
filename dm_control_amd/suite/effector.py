"""End-effector velocity observations for the device-resident environments: `wrap(env, targets, ...)`.

The twin of `suite/proximity.py` for `jacobian.BatchJacobian`: where the reference calls `mj_objectVelocity` once per
object of one environment on the host (mujoco/wrapper/core.py:522) or declares velocimeter / frame sensors in the model,
the wrapper enqueues one `BatchJacobian.velocity()` launch on the environment's stream after every step and reset and
returns the targets' 6D velocities -- a (B, 6 T) tensor in the batch precision, per target (angular, linear) -- as, or
in, the observation.  Nothing is read back to the host and the model is not edited.

The velocities are J qvel at the qpos and qvel in device memory: no pose array is read, so the environment's output mask
and a recorded HIP graph stay as they are.
"""
from dm_control_amd import jacobian as jacobian_lib
from dm_control_amd.suite import observation_wrapper


class EffectorEnv(observation_wrapper.ObservationWrapper):
  """An environment whose observations are (or include) target velocities; everything else is the wrapped environment's."""
  _ONLY = 'effector_only'

  def __init__(self, env, targets, observation_key='effector_velocity', effector_only=False, local=False):
    if not list(targets):
      raise ValueError('targets: at least one target is needed')
    super().__init__(env, observation_key, effector_only)
    self.local = bool(local)
    self.jacobian = jacobian_lib.BatchJacobian(env, targets)      # (no _require_outputs: the unit reads qpos and qvel alone)

  def read(self):
    """The (B, 6 T) velocities of the state in device memory, enqueued on the current stream."""
    v = self.jacobian.velocity(local=self.local)
    return v.reshape(v.shape[0], -1)

  def _read(self):
    return self.read()


def wrap(env, targets, observation_key='effector_velocity', effector_only=False, local=False):
  """env: a `fused_env` / `torch_env` / `device_env` / `composer.make` environment; targets: a list of
  `jacobian.BatchJacobian` targets (a site name, dict(body=..[, com=True | offset=..]), dict(geom=..)); local: the
  velocities in each target's own frame instead of the world's."""
  return EffectorEnv(env, targets, observation_key, effector_only, local)

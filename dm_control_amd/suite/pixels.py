"""Pixel observations for the device-resident environments: `wrap(env, cameras, ...)`.

The counterpart of the reference's `suite/wrappers/pixels.py` (which calls `physics.render` on the host, one
environment at a time) for `fused_env`, `torch_env`, `device_env` and `composer.make(...)` environments: after every
step and reset the wrapper enqueues one `camera.BatchCamera` render on the environment's stream and returns the image
tensor -- (B, C, H, W, 3) uint8 RGB, (B, C, H, W) depth or (B, C, H, W, 2) int32 segmentation -- as the observation.
Nothing is read back to the host.  The images are the geometric camera's (see camera.py), not OpenGL's.
"""
from dm_control_amd import camera as camera_lib
from dm_control_amd.suite import observation_wrapper

_KINDS = ('rgb', 'depth', 'segmentation')


class PixelEnv(observation_wrapper.ObservationWrapper):
  """An environment whose observations are (or include) camera images; everything else is the wrapped environment's."""
  _ONLY = 'pixels_only'

  def __init__(self, env, cameras, height=84, width=84, kind='rgb', pixels_only=True, observation_key='pixels', **camera_kwargs):
    if kind not in _KINDS:
      raise ValueError('kind must be one of %s' % (_KINDS,))
    super().__init__(env, observation_key, pixels_only)
    self.kind = kind
    self.camera = camera_lib.BatchCamera(env, cameras, height, width, **camera_kwargs)
    self._require_outputs(self.camera)

  def render(self):
    """The image of the state in device memory, enqueued on the current stream."""
    return self.camera.render(depth=self.kind == 'depth', segmentation=self.kind == 'segmentation')

  def _read(self):
    return self.render()


def wrap(env, cameras, height=84, width=84, kind='rgb', pixels_only=True, **kwargs):
  """env: a `fused_env` / `torch_env` / `device_env` / `composer.make` environment; cameras: names or ids of the model's
  cameras (e.g. 'home0/egocentric') or user specs (camera.resolve_camera)."""
  return PixelEnv(env, cameras, height, width, kind, pixels_only, **kwargs)

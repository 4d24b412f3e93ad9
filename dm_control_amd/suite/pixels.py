"""Pixel observations for the device-resident environments: `wrap(env, cameras, ...)`.

The counterpart of the reference's `suite/wrappers/pixels.py` (which calls `physics.render` on the host, one
environment at a time) for `fused_env`, `torch_env`, `device_env` and `composer.make(...)` environments: after every
step and reset the wrapper enqueues one `camera.BatchCamera` render on the environment's stream and returns the image
tensor -- (B, C, H, W, 3) uint8 RGB, (B, C, H, W) depth or (B, C, H, W, 2) int32 segmentation -- as the observation.
Nothing is read back to the host.  The images are the geometric camera's (see camera.py), not OpenGL's.
"""
from dm_control_amd import camera as camera_lib

_KINDS = ('rgb', 'depth', 'segmentation')


class PixelEnv:
  """An environment whose observations are (or include) camera images; everything else is the wrapped environment's."""

  def __init__(self, env, cameras, height=84, width=84, kind='rgb', pixels_only=True, observation_key='pixels', **camera_kwargs):
    if kind not in _KINDS:
      raise ValueError('kind must be one of %s' % (_KINDS,))
    self.env = env
    self.kind, self.pixels_only, self.observation_key = kind, bool(pixels_only), observation_key
    self.camera = camera_lib.BatchCamera(env, cameras, height, width, **camera_kwargs)
    batch = self.camera.batch
    # the step launches must write the poses the cameras read; a recorded HIP graph keeps the mask it was captured with
    need = batch.output_mask | self.camera.output_mask
    if need != batch.output_mask:
      batch.set_output_mask(need)
    if getattr(env, 'output_mask', None) is not None:
      env.output_mask |= self.camera.output_mask      # (fused_env restores this mask after drawing start states)
    if hasattr(env, 'invalidate_graph'):
      env.invalidate_graph()
    elif getattr(env, '_graph', None) is not None:
      raise ValueError('wrap the environment before recording its control step into a HIP graph (capture_graph): the '
                       'recorded launches write the derived arrays of the output mask they were captured with')
    self._out = None

  def __getattr__(self, name):
    return getattr(self.env, name)

  def render(self):
    """The image of the state in device memory, enqueued on the current stream."""
    return self.camera.render(depth=self.kind == 'depth', segmentation=self.kind == 'segmentation')

  def _observe(self, result):
    img = self.render()
    if hasattr(result, '_replace') and hasattr(result, 'observation'):      # a TimeStep (composer)
      obs = {} if self.pixels_only else dict(result.observation)
      obs[self.observation_key] = img
      return result._replace(observation=obs)
    if isinstance(result, tuple):      # (obs, reward, done, ...)
      return ((img if self.pixels_only else {'state': result[0], self.observation_key: img}),) + tuple(result[1:])
    return img if self.pixels_only else {'state': result, self.observation_key: img}

  def step(self, action=None):
    return self._observe(self.env.step(action))

  def reset(self, *args, **kwargs):
    return self._observe(self.env.reset(*args, **kwargs))


def wrap(env, cameras, height=84, width=84, kind='rgb', pixels_only=True, **kwargs):
  """env: a `fused_env` / `torch_env` / `device_env` / `composer.make` environment; cameras: names or ids of the model's
  cameras (e.g. 'home0/egocentric') or user specs (camera.resolve_camera)."""
  return PixelEnv(env, cameras, height, width, kind, pixels_only, **kwargs)

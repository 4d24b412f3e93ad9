"""ObservationWrapper: the base of the wrappers that add a batch unit's output to an environment's observations
(`pixels.PixelEnv`, `lidar.LidarEnv`).  A derived class creates its unit, calls `_require_outputs` on it, says what one
observation is (`_read`) and names its own "only" attribute (`_ONLY`); stepping, resetting and merging are here."""


class ObservationWrapper:
  """An environment whose observations are (or include, under `observation_key`) what `_read()` returns; everything else
  is the wrapped environment's."""

  _ONLY = None      # the attribute that says whether the observation is `_read()` alone, e.g. 'pixels_only'

  def __init__(self, env, observation_key, only):
    self.env, self.observation_key = env, observation_key
    setattr(self, self._ONLY, bool(only))

  def _require_outputs(self, unit):
    """The step launches must write the poses the unit reads; a recorded HIP graph keeps the mask it was captured with."""
    env, batch = self.env, unit.batch
    need = batch.output_mask | unit.output_mask
    if need != batch.output_mask:
      batch.set_output_mask(need)
    if getattr(env, 'output_mask', None) is not None:
      env.output_mask |= unit.output_mask      # (fused_env restores this mask after drawing start states)
    if hasattr(env, 'invalidate_graph'):
      env.invalidate_graph()
    elif getattr(env, '_graph', None) is not None:
      raise ValueError('wrap the environment before recording its control step into a HIP graph (capture_graph): the '
                       'recorded launches write the derived arrays of the output mask they were captured with')

  def __getattr__(self, name):
    return getattr(self.env, name)

  def _observe(self, result):
    value, only = self._read(), getattr(self, self._ONLY)
    if hasattr(result, '_replace') and hasattr(result, 'observation'):      # a TimeStep (composer)
      obs = {} if only else dict(result.observation)
      obs[self.observation_key] = value
      return result._replace(observation=obs)
    if isinstance(result, tuple):      # (obs, reward, done, ...)
      return ((value if only else {'state': result[0], self.observation_key: value}),) + tuple(result[1:])
    return value if only else {'state': result, self.observation_key: value}

  def step(self, action=None):
    return self._observe(self.env.step(action))

  def reset(self, *args, **kwargs):
    return self._observe(self.env.reset(*args, **kwargs))

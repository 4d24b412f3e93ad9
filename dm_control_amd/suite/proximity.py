"""Proximity observations for the device-resident environments: `wrap(env, pairs, distmax, ...)`.

The twin of `suite/lidar.py` for geom distances: where the reference needs one `<distance>` sensor per pair in the model
(and reads `sensordata` on the host), the wrapper enqueues one `distance.BatchDistance` query on the environment's stream
after every step and reset and returns the signed distances -- a (B, P) tensor in the batch precision -- as, or in, the
observation.  Nothing is read back to the host and the model is not edited.

A pair farther apart than `distmax` reads distmax; overlapping geoms read minus their penetration depth.
`scale='tanh'` squashes on the device instead: tanh(dist / distmax), in (-1, tanh(1)]; it needs a finite positive distmax.
"""
import numpy as np

from dm_control_amd import distance as distance_lib
from dm_control_amd.suite import observation_wrapper

_SCALES = (None, 'tanh')


class ProximityEnv(observation_wrapper.ObservationWrapper):
  """An environment whose observations are (or include) geom distances; everything else is the wrapped environment's."""
  _ONLY = 'proximity_only'

  def __init__(self, env, pairs, distmax, observation_key='proximity', proximity_only=False, scale=None, **distance_kwargs):
    if scale not in _SCALES:
      raise ValueError('scale must be one of %s' % (_SCALES,))
    dm = np.asarray(distmax, dtype=np.float64)
    if scale == 'tanh' and not (np.all(np.isfinite(dm)) and np.all(dm > 0)):
      raise ValueError("scale='tanh' divides by distmax: give a finite positive one")
    if not list(pairs):
      raise ValueError('pairs: at least one pair is needed')
    super().__init__(env, observation_key, proximity_only)
    self.scale = scale
    self.distance = distance_lib.BatchDistance(env, pairs, distmax=distmax, **distance_kwargs)
    self._require_outputs(self.distance)
    self._distmax = None

  def read(self):
    """The (B, P) distances of the state in device memory, enqueued on the current stream."""
    import torch      # pylint: disable=import-outside-toplevel
    dist = self.distance.query()
    if self.scale == 'tanh':
      if self._distmax is None:
        self._distmax = torch.as_tensor(self.distance.distmax, dtype=dist.dtype, device=dist.device)
      dist = torch.tanh(dist / self._distmax)
    return dist

  def _read(self):
    return self.read()


def wrap(env, pairs, distmax, observation_key='proximity', proximity_only=False, scale=None, **kw):
  """env: a `fused_env` / `torch_env` / `device_env` / `composer.make` environment; pairs: [(member1, member2), ...] with a
  member a geom name, a geom id or dict(body=..) (distance.resolve_member); distmax: one cutoff or one per pair.
  kw: BatchDistance's tolerance / iterations."""
  return ProximityEnv(env, pairs, distmax, observation_key, proximity_only, scale, **kw)

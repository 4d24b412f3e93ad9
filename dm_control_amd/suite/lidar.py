"""Range-scan ("lidar") observations for the device-resident environments: `wrap(env, frame, directions, ...)`.

The twin of `suite/pixels.py` for rays: where the reference needs one `<site>` and one `<rangefinder>` per ray in the
model (and reads `sensordata` on the host), the wrapper enqueues one `rays.BatchRays` scan on the environment's stream
after every step and reset and returns the distances -- a (B, R) tensor in the batch precision -- as, or in, the
observation.  Nothing is read back to the host and the model is not edited.

Directions are normalised, so a distance is in metres; a ray that hits nothing (or nothing within `cutoff`) reads -1, the
rangefinder's value.  `scale='tanh'` squashes on the device instead: tanh(dist / cutoff), in [0, tanh(1)] for a hit, and a
miss is mapped to 1 -- farther than anything that was hit; it needs a `cutoff`.  The rays skip the body the frame belongs
to, as a rangefinder skips its site's body (`bodyexclude` overrides).
"""
import numpy as np

from dm_control_amd import rays as rays_lib
from dm_control_amd.suite import observation_wrapper

_SCALES = (None, 'tanh')


class LidarEnv(observation_wrapper.ObservationWrapper):
  """An environment whose observations are (or include) a range scan; everything else is the wrapped environment's."""
  _ONLY = 'lidar_only'

  def __init__(self, env, frame, directions, observation_key='lidar', lidar_only=False, cutoff=None, scale=None,
               offset=(0, 0, 0), bodyexclude='frame', **rays_kwargs):
    if scale not in _SCALES:
      raise ValueError('scale must be one of %s' % (_SCALES,))
    if scale == 'tanh' and cutoff is None:
      raise ValueError("scale='tanh' divides by the cutoff: give one")
    d = np.asarray(directions, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 3 or d.shape[0] < 1:
      raise ValueError('directions: expected an (R, 3) array')
    n = np.linalg.norm(d, axis=1, keepdims=True)
    if not np.all(n > 0):
      raise ValueError('directions: a direction has zero length')
    super().__init__(env, observation_key, lidar_only)
    self.scale = scale
    self.rays = rays_lib.BatchRays(env, cutoff=cutoff, **rays_kwargs)
    self.rays.add_scan(frame, d / n, offset=offset, bodyexclude=bodyexclude)
    self._require_outputs(self.rays)

  def scan(self):
    """The (B, R) scan of the state in device memory, enqueued on the current stream."""
    import torch      # pylint: disable=import-outside-toplevel
    dist = self.rays.scan()[0][:, 0]
    if self.scale == 'tanh':
      dist = torch.where(dist < 0, torch.ones_like(dist), torch.tanh(dist / self.rays.cutoff))
    return dist

  def _read(self):
    return self.scan()


def wrap(env, frame, directions, observation_key='lidar', lidar_only=False, cutoff=None, scale=None, **kw):
  """env: a `fused_env` / `torch_env` / `device_env` / `composer.make` environment; frame: 'world', dict(body=..),
  dict(site=..), dict(geom=..) or dict(camera=..) (rays.resolve_frame); directions: (R, 3) in that frame, e.g.
  `rays.ring(64)`.  kw: offset, bodyexclude, and BatchRays' geomgroup / flg_static."""
  return LidarEnv(env, frame, directions, observation_key, lidar_only, cutoff, scale, **kw)

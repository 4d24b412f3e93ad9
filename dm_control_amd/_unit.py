"""BatchUnit: what the add-on units of a batch share on the host -- camera.BatchCamera, rays.BatchRays and
utils.inverse_kinematics.BatchIK, each a native object created against a `BatchedPhysics` that launches on a torch stream
and returns torch tensors on the batch's device.  A new unit derives from it and keeps only what is its own."""
import logging

from dm_control_amd import _native

PRIMITIVE_TYPES = (0, 2, 3, 4, 5, 6)      # plane, sphere, capsule, ellipsoid, cylinder, box: camera_core.h cam_primitive


def find_batch(obj, depth=3):
  """The BatchedPhysics inside a Physics / environment object, or None."""
  if hasattr(obj, 'device_ptr') and hasattr(obj, 'set_output_mask') and hasattr(obj, 'model'):
    return obj
  if depth > 0:
    for attr in ('batch', 'host_physics', 'physics'):
      try:
        sub = getattr(obj, attr, None)
      except Exception:  # pylint: disable=broad-except
        sub = None
      if sub is not None and sub is not obj:
        found = find_batch(sub, depth - 1)
        if found is not None:
          return found
  return None


def skipped_geoms(model, who):
  """The mesh / height-field geoms (names, or ids where unnamed): scenery no ray of the cameras or of the ray casts hits."""
  names = model.names.get('geom', [None] * model.ngeom)
  skipped = [names[g] if names[g] is not None else g for g in range(model.ngeom) if int(model.geom_type[g]) not in PRIMITIVE_TYPES]
  if skipped:
    logging.getLogger(__name__).info('%s: %d mesh / height-field geoms are not ray-cast: %s', who, len(skipped), skipped)
  return skipped


class BatchUnit:
  """A native object (`_ptr`) that lives on `self.batch`; a derived class names the C symbol that destroys it."""
  _DESTROY = None
  _OUT_ERROR = 'out must be a contiguous %s tensor of shape %s on %s'
  _ptr = None

  def close(self):
    if self._ptr:
      getattr(_native.lib(), self._DESTROY)(self._ptr)
      self._ptr = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  def _torch(self):
    """(torch, the batch's device, the dtype of its reals)"""
    import torch      # pylint: disable=import-outside-toplevel
    return torch, torch.device('cuda', self.batch.device_id), torch.float64 if int(self.batch.precision) == 64 else torch.float32

  def stream_handle(self, stream):
    """The raw handle of `stream` (a torch stream or a handle); None: torch's current stream on the batch's device."""
    if stream is None:
      torch, dev, _ = self._torch()
      return torch.cuda.current_stream(dev).cuda_stream or None
    return getattr(stream, 'cuda_stream', stream) or None

  def _tensor(self, shape, dtype, out=None):
    """`out` if it is a contiguous tensor of that shape and dtype on the batch's device (ValueError otherwise), or a new one."""
    torch, dev, _ = self._torch()
    if out is None:
      return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
      raise ValueError(self._OUT_ERROR % (dtype, tuple(shape), dev))
    return out

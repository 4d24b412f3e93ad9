"""BatchDistance: mj_geomDistance for a whole batch -- the signed distance between pairs of geoms, the closest points and
the normal, computed on the device by one HIP launch.

The reference asks one pair of one environment per call (`mujoco.mj_geomDistance`) or declares `<distance>`, `<normal>`
and `<fromto>` sensors in the model (dm_control/mjcf/schema.xml:3047-3095).  This module gives a batch the same numbers as
tensors that never leave the GPU:

  * a pair is (member1, member2); a member is a geom name, a geom id or `dict(body=...)` (a name or an id): every geom
    directly attached to that body, the pair's answer being the minimum over the geom pairs -- the sensors' body1 / body2.
  * dist: the Euclidean distance when the geoms are apart, minus the minimum-translation depth when they overlap;
    fromto: the point on member1's surface and the point on member2's that realise it; normal = (to - from) / dist, from
    member1 towards member2 when apart.
  * `distmax` (one value or one per pair; default: infinity) bounds the result: a pair with no distance below it reads
    distmax (inf under the default: plane-plane, for one), a zero fromto and a zero normal -- mj_geomDistance's rule.  Planes are infinite; plane-plane has no distance (distmax).
  * mesh and height-field geoms are refused by name (`unsupported_geoms` lists the model's).
  * witness points are not unique for parallel faces or edges; which are returned is the solver's choice.

Poses are the geom_xpos / geom_xmat the last step or forward launch wrote; geom sizes are the ones the step kernel uses
(after `set_model_real`, and per environment for `set_env_geoms` geoms).  The solver is GJK on the geoms' cores (a sphere
is a point plus a radius, a capsule a segment plus a radius) and EPA where the cores overlap: csrc/dist_core.h.
"""
import ctypes
import xml.etree.ElementTree as ET

import numpy as np

from dm_control_amd import _native
from dm_control_amd import _unit

SUPPORTED_TYPES = _unit.PRIMITIVE_TYPES
KINDS = ('distance', 'normal', 'fromto')


class _Options(ctypes.Structure):      # dmc_dist_options
  _fields_ = [('tolerance', ctypes.c_double), ('iterations', ctypes.c_int32), ('reserved', ctypes.c_int32)]


def unsupported_geoms(model):
  """The mesh / height-field geoms of the model (names, or ids where unnamed): no pair may hold one."""
  names = model.names.get('geom', [None] * model.ngeom)
  return [names[g] if names[g] is not None else g for g in range(model.ngeom) if int(model.geom_type[g]) not in SUPPORTED_TYPES]


def resolve_member(model, member):
  """The geom ids a pair member stands for: [id] for a geom name or id, the geoms directly attached to the body for
  dict(body=name or id)."""
  names = model.names.get('geom', [None] * model.ngeom)
  if isinstance(member, dict):
    if len(member) != 1 or next(iter(member)) not in ('body', 'geom'):
      raise ValueError('pair member: expected a geom name, a geom id, dict(geom=..) or dict(body=..), got %r' % (member,))
    kind, key = next(iter(member.items()))
    if kind == 'geom':
      return resolve_member(model, key)
    b = model.name2id(key, 'body') if isinstance(key, str) else int(key)
    if not 0 <= b < model.nbody:
      raise ValueError('pair member: body id %d out of range (the model has %d bodies)' % (b, model.nbody))
    ids = [g for g in range(model.ngeom) if int(model.geom_bodyid[g]) == b]
    if not ids:
      raise ValueError('pair member: body %r has no geoms directly attached to it' % (key,))
  elif isinstance(member, str):
    ids = [model.name2id(member, 'geom')]
  elif isinstance(member, (int, np.integer)):
    ids = [int(member)]
    if not 0 <= ids[0] < model.ngeom:
      raise ValueError('pair member: geom id %d out of range (the model has %d geoms)' % (ids[0], model.ngeom))
  else:
    raise ValueError('pair member: expected a geom name, a geom id, dict(geom=..) or dict(body=..), got %r' % (member,))
  bad = [names[g] if names[g] is not None else g for g in ids if int(model.geom_type[g]) not in SUPPORTED_TYPES]
  if bad:
    raise ValueError('pair member %r: mesh / height-field geoms have no distance: %s' % (member, bad))
  return ids


def pair_tables(model, pairs, distmax):
  """(pair_adr (P, 4) int32, member (M,) int32, distmax (P,) float64) of a pair list, as dmc_dist_create takes them."""
  pairs = list(pairs)
  if not pairs:
    raise ValueError('pairs: at least one pair is needed')
  adr, member = [], []
  for p in pairs:
    if not isinstance(p, (tuple, list)) or len(p) != 2:
      raise ValueError('pairs: each pair is (member1, member2), got %r' % (p,))
    row = []
    for side in p:
      ids = resolve_member(model, side)
      row += [len(member), len(ids)]
      member += ids
    adr.append(row)
  dm = np.asarray(distmax, dtype=np.float64)
  if dm.ndim not in (0, 1) or (dm.ndim == 1 and dm.shape[0] != len(pairs)):
    raise ValueError('distmax: one value, or one per pair (%d), got shape %s' % (len(pairs), dm.shape))
  if np.any(np.isnan(dm)):
    raise ValueError('distmax is NaN')
  return (np.ascontiguousarray(adr, dtype=np.int32), np.ascontiguousarray(member, dtype=np.int32),
          np.ascontiguousarray(np.broadcast_to(dm, (len(pairs),)), dtype=np.float64))


def pairs_from_sensors(xml_string):
  """The <distance>, <normal> and <fromto> sensor elements of an MJCF string as dict(pairs, distmax, kinds, names): what
  to hand to `BatchDistance` (the compiler refuses these elements in a model: they would change `sensordata`).  A sensor
  names geom1 or body1 and geom2 or body2; cutoff (default 0) is mj_geomDistance's distmax, as in MuJoCo's sensor."""
  root = ET.fromstring(xml_string)
  pairs, cut, kinds, names = [], [], [], []
  for sensor in root.iter('sensor'):
    for e in sensor:
      if e.tag not in KINDS:
        continue
      sides = []
      for k in ('1', '2'):
        g, b = e.get('geom' + k), e.get('body' + k)
        if (g is None) == (b is None):
          raise ValueError('sensor <%s name=%r>: exactly one of geom%s / body%s is needed' % (e.tag, e.get('name'), k, k))
        sides.append(g if g is not None else dict(body=b))
      pairs.append(tuple(sides))
      cut.append(float(e.get('cutoff', 0)))
      kinds.append(e.tag)
      names.append(e.get('name'))
  return dict(pairs=pairs, distmax=np.array(cut), kinds=kinds, names=names)


class BatchDistance(_unit.BatchUnit):
  """Geom distances for every environment of a batch; see the module docstring.

  physics_or_batch: a `BatchedPhysics`, or anything holding one as `.batch` (Physics) or `.physics`.
  pairs: [(member1, member2), ...]; distmax: one cutoff or one per pair; tolerance, iterations: mjOption's ccd_tolerance
  and ccd_iterations (defaults 1e-6, 50).  These are fixed for the object's life.
  """
  _DESTROY = 'dmc_dist_destroy'
  _OUT_ERROR = 'out: expected a contiguous %s tensor of shape %s on %s'

  def __init__(self, physics_or_batch, pairs, distmax=np.inf, tolerance=1e-6, iterations=50):
    if not 0 < float(tolerance) < 1:
      raise ValueError('tolerance must lie in (0, 1)')
    if int(iterations) < 1:
      raise ValueError('iterations must be positive')
    batch = _unit.find_batch(physics_or_batch)
    if batch is None:
      raise TypeError('BatchDistance needs a BatchedPhysics (or an object holding one as .batch / .physics / .host_physics)')
    self.batch, self.model = batch, batch.model
    self.pairs = list(pairs)
    self.pair_adr, self.member, self.distmax = pair_tables(self.model, self.pairs, distmax)
    self.tolerance, self.iterations = float(tolerance), int(iterations)
    self.skipped_geoms = unsupported_geoms(self.model)      # what no pair may name: the unit's gap
    opt = _Options(self.tolerance, self.iterations, 0)
    self._ptr = ctypes.c_void_p()
    _native.check(_native.lib().dmc_dist_create(batch._ptr, len(self.pairs), self.pair_adr.ctypes.data, self.member.ctypes.data,
                                                len(self.member), self.distmax.ctypes.data, ctypes.byref(opt), ctypes.byref(self._ptr)))
    from dm_control_amd.batch import OUT      # pylint: disable=import-outside-toplevel
    self.output_mask = OUT['geom']      # the derived arrays a step launch must write for this unit

  def info(self):
    a = np.zeros(10, dtype=np.int32)
    _native.check(_native.lib().dmc_dist_info(self._ptr, a.ctypes.data))
    return dict(zip(('B', 'precision', 'npair', 'nmember', 'iterations', 'block', 'epa_vertices', 'epa_faces', 'epa_lanes_per_pass',
                     'lds_bytes'), (int(x) for x in a)))

  def query(self, fromto=False, normal=False, status=False, out=None, stream=None):
    """Every pair of every environment in one launch.  Returns dist (B, P) in the batch precision, or a tuple (dist[,
    fromto (B, P, 6)][, normal (B, P, 3)][, status (B, P) int32]) of what was asked for.  status: 0 converged, 1 a cap
    (iterations, polytope size) was reached and dist is the best bound found; status='bits' returns the kernel's word
    (bit 0 that flag, bit 1 set when a geom pair's cores overlapped and EPA ran).  Asynchronous on `stream` (a torch stream
    or a raw handle; default: torch's current stream), capturable in a HIP graph; `out`, a sequence of such tensors in the
    same order, is written in place.  The host is never read."""
    torch, _, dt = self._torch()
    shape = (self.batch.batch_size, len(self.pairs))
    want = [(shape, dt)] + ([(shape + (6,), dt)] if fromto else []) + ([(shape + (3,), dt)] if normal else []) + \
           ([(shape, torch.int32)] if status else [])
    out = [None] * len(want) if out is None else ([out] if isinstance(out, torch.Tensor) else list(out))
    if len(out) != len(want):
      raise ValueError('out must hold %d tensors (dist%s%s%s)' % (len(want), ', fromto' if fromto else '', ', normal' if normal else '',
                                                                  ', status' if status else ''))
    res = [self._tensor(s, d, o) for (s, d), o in zip(want, out)]
    it = iter(res[1:])
    ft = next(it) if fromto else None
    nr = next(it) if normal else None
    st = next(it) if status else None
    _native.check(_native.lib().dmc_dist_query(self._ptr, res[0].data_ptr(), ft.data_ptr() if fromto else None,
                                               nr.data_ptr() if normal else None, st.data_ptr() if status else None,
                                               self.stream_handle(stream)))
    if status and status != 'bits':
      st.bitwise_and_(1)
    return res[0] if len(res) == 1 else tuple(res)

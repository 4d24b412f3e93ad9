"""BatchContacts: the contact wrench of every contact and the net contact force on bodies and geom sets for a whole batch,
each computed on the device by one HIP launch.

The reference asks one contact of one environment per call (`mj_contactForce`, mujoco/wrapper/core.py:527-552), and a task
that wants "the ground reaction force on each foot" loops over `mjData.contact` on the host or adds `<touch>` sensors to
the model.  This module gives a batch the same numbers as tensors that never leave the GPU:

  * a target is a set of geoms S and an optional filter O on the partner geom: a geom name or id (a bare string or int),
    `dict(geom=..)`, `dict(body=..)` (the body's own geoms) or `dict(body=.., subtree=True)` (the body and everything below
    it), each with `other=<the same forms>` (default: every geom).  Names, ids or lists of them.
  * contact c < ncon between geom1 and geom2, with the contact-frame force lf ("contact_force") and the frame F
    ("contact_frame", rows normal, tangent, tangent), pushes geom2's body with f_c = F' lf[0:3] and the torque
    t_c = F' lf[3:6] about the contact point; geom1's body receives the opposite.  It counts for a target with s = +1 when
    geom2 is in S, geom1 in O and geom1 not in S; with s = -1 when geom1 is in S, geom2 in O and geom2 not in S.  Contacts
    with both geoms in S are internal and skipped.
  * wrench():  (B, nconmax, 6) = [f_c, t_c] of every contact slot, zeros past the environment's ncon.
  * net():     force, torque (B, T, 3): sum of s f_c and of s (t_c + (p_c - r) x f_c), r the named body's xipos
               (`about='com'`), xpos ('origin') or 0 ('world'); `local` rotates both into the named body's frame.  The
               named body is the target's body, or its geom's body.
  * normal():  (B, T) sum of lf[0] over the counted contacts: what a touch sensor on the set reads; >= 0.
  * count():   (B, T) int32, the counted contacts;  dist(): (B, T) the smallest contact_dist among them, +inf: none.
  * net_all(): the five of them from one launch.

The contacts are visited in index order by one lane in plain arithmetic: two launches give equal bits.

VALIDITY.  The unit reads what the LAST launch wrote.  The contact arrays are consistent with each other and with the
state after `forward()`, `step(forward_after=True)`, `step2`, and after a non-legacy `step` (the values of the last
step's start state, as in MuJoCo).  After a PLAIN LEGACY STEP they are not: the launch ends with a partial mj_step1 that
re-runs the collision without the constraints, so the contact list is new and the forces are those of the step's start.
`refresh()` enqueues the missing forward without moving the solver's warm start; call it before reading after a plain
legacy step.
"""
import ctypes

import numpy as np

from dm_control_amd import _native
from dm_control_amd import _unit
from dm_control_amd import batch as batch_lib
from dm_control_amd import host_data

MAX_TARGETS = 64
ABOUT = host_data.CONTACT_ABOUT
_ABOUT_OUT = {'com': batch_lib.OUT['xipos'], 'origin': batch_lib.OUT['xpos'], 'world': 0}
OUTPUTS = ('force', 'torque', 'normal', 'count', 'dist')


class _Tables(ctypes.Structure):      # dmc_con_tables
  _fields_ = [('ntarget', ctypes.c_int32), ('ngeom', ctypes.c_int32), ('words', ctypes.c_int32), ('about', ctypes.c_int32),
              ('body', ctypes.c_void_p), ('masks', ctypes.c_void_p)]


def pack_mask(mask):
  """A (ngeom,) bool mask as ceil(ngeom / 32) uint32 words: bit g is bit g % 32 of word g // 32."""
  mask = np.asarray(mask, dtype=bool)
  words = np.zeros((mask.size + 31)//32, dtype=np.uint32)
  for g in np.nonzero(mask)[0]:
    words[g >> 5] |= np.uint32(1 << (int(g) & 31))
  return words


def target_tables(model, targets, about='com'):
  """dict(body (T,) int32, masks (T, 2, words) uint32, about, resolved) of a target list, as dmc_con_create takes them."""
  if about not in ABOUT:
    raise ValueError('about must be one of %s, got %r' % (ABOUT, about))
  resolved = host_data.contact_targets(model, targets)
  if len(resolved) > MAX_TARGETS:
    raise ValueError('targets: %d targets, at most %d per object' % (len(resolved), MAX_TARGETS))
  masks = np.ascontiguousarray([[pack_mask(d['S']), pack_mask(d['O'])] for d in resolved], dtype=np.uint32)
  return dict(body=np.ascontiguousarray([d['body'] for d in resolved], dtype=np.int32), masks=masks, about=ABOUT.index(about),
              resolved=resolved)


class BatchContacts(_unit.BatchUnit):
  """Contact wrenches and net contact forces for every environment of a batch; see the module docstring.

  physics_or_batch: a `BatchedPhysics`, or anything holding one as `.batch` (Physics) or `.physics`.
  targets: a list of targets (T <= 64); about: 'com' | 'origin' | 'world'; local: the default of `net` / `net_all`.
  These are fixed for the object's life.  `output_mask` names the step outputs the unit reads.  The batch's field
  pointers are read at every call, so fields rebound with `bind` are followed.
  """
  _DESTROY = 'dmc_con_destroy'
  _OUT_ERROR = 'out: expected a contiguous %s tensor of shape %s on %s'

  def __init__(self, physics_or_batch, targets, about='com', local=False):
    batch = _unit.find_batch(physics_or_batch)
    if batch is None:
      raise TypeError('BatchContacts needs a BatchedPhysics (or an object holding one as .batch / .physics / .host_physics)')
    self.batch, self.model = batch, batch.model
    self.about, self.local = about, bool(local)
    self.tables = target_tables(self.model, targets, about)
    self.targets = list(targets) if isinstance(targets, (list, tuple)) else [targets]
    self.output_mask = self._need(True, self.local)
    masks, body = self.tables['masks'], self.tables['body']
    tb = _Tables(len(body), self.model.ngeom, masks.shape[2], self.tables['about'], body.ctypes.data, masks.ctypes.data)
    self._ptr = ctypes.c_void_p()
    _native.check(_native.lib().dmc_con_create(batch._ptr, ctypes.byref(tb), ctypes.byref(self._ptr)))
    self.nconmax = self.info()['nconmax']

  def _need(self, torque, rotate):
    return batch_lib.OUT['contact'] | (_ABOUT_OUT[self.about] if torque else 0) | (batch_lib.OUT['xmat'] if rotate else 0)

  def _require(self, need):
    if (int(self.batch.output_mask) & need) != need:
      raise ValueError('BatchContacts: the batch\'s output mask (0x%x) lacks arrays this call reads (0x%x): the contact arrays '
                       '(OUT["contact"]) and the poses `about` / `local` need' % (int(self.batch.output_mask), need))

  @property
  def shape(self):
    """(B, T)"""
    return self.batch.batch_size, len(self.tables['body'])

  def info(self):
    a = np.zeros(8, dtype=np.int32)
    _native.check(_native.lib().dmc_con_info(self._ptr, a.ctypes.data))
    return dict(zip(('B', 'precision', 'ntarget', 'nconmax', 'block', 'words', 'lds_bytes', 'output_mask'), (int(x) for x in a)))

  def wrench(self, out=None, stream=None):
    """(B, nconmax, 6) = [f_c, t_c] of every contact slot in the world frame, the force on geom2's body and the torque about
    the contact point; zeros past the environment's ncon.  One launch, asynchronous on `stream` (a torch stream or a raw
    handle; default: torch's current stream), capturable in a HIP graph; `out` is written in place.  Every element is
    written.  The host is never read."""
    _, _, dt = self._torch()
    self._require(batch_lib.OUT['contact'])
    res = self._tensor((self.batch.batch_size, self.nconmax, 6), dt, out)
    _native.check(_native.lib().dmc_con_wrench(self._ptr, res.data_ptr(), self.stream_handle(stream)))
    return res

  def _launch(self, names, local, out, stream):
    torch, _, dt = self._torch()
    B, T = self.shape
    local = self.local if local is None else bool(local)
    self._require(self._need('torque' in names, local and ('force' in names or 'torque' in names)))
    shapes = dict(force=((B, T, 3), dt), torque=((B, T, 3), dt), normal=((B, T), dt), count=((B, T), torch.int32), dist=((B, T), dt))
    out = out or {}
    res = {k: self._tensor(shapes[k][0], shapes[k][1], out.get(k)) for k in names}
    ptr = lambda k: res[k].data_ptr() if k in res else None
    _native.check(_native.lib().dmc_con_net(self._ptr, int(local), ptr('force'), ptr('torque'), ptr('normal'), ptr('count'),
                                            ptr('dist'), self.stream_handle(stream)))
    return res

  def net(self, local=None, out=None, stream=None):
    """(force, torque), each (B, T, 3): the net contact force on every target and its torque about r (`about`), in the world
    frame or (`local`; default: the object's) the named body's.  One launch; `out`: the pair; `stream` as in `wrench`."""
    if out is not None:
      if len(out) != 2:
        raise ValueError('out must hold 2 tensors (force, torque)')
      out = dict(force=out[0], torque=out[1])
    r = self._launch(('force', 'torque'), local, out, stream)
    return r['force'], r['torque']

  def normal(self, out=None, stream=None):
    """(B, T): the sum of the normal forces of the counted contacts, what a touch sensor on the set reads.  One launch."""
    return self._launch(('normal',), False, None if out is None else dict(normal=out), stream)['normal']

  def count(self, out=None, stream=None):
    """(B, T) int32: the number of counted contacts.  One launch."""
    return self._launch(('count',), False, None if out is None else dict(count=out), stream)['count']

  def dist(self, out=None, stream=None):
    """(B, T): the smallest contact distance among the counted contacts, +inf where there is none.  One launch."""
    return self._launch(('dist',), False, None if out is None else dict(dist=out), stream)['dist']

  def net_all(self, local=None, out=None, stream=None):
    """dict(force, torque, normal, count, dist) from ONE launch; `out`: a dict with any of them to write in place."""
    return self._launch(OUTPUTS, local, out, stream)

  def refresh(self, stream=None):
    """Makes the contact arrays consistent with the state in device memory: a forward launch bracketed by device-to-device
    copies of qacc_warmstart into a buffer the object owns and back -- a query must not move the solver's warm start -- and
    the batch's stashes invalidated.  Asynchronous on `stream`, no host sync.  Only needed after a plain legacy step."""
    L, h = _native.lib(), self.stream_handle(stream)
    _native.check(L.dmc_con_warmstart(self._ptr, 0, h))
    self.batch.forward(stream=h)
    _native.check(L.dmc_con_warmstart(self._ptr, 1, h))
    _native.check(L.dmc_batch_invalidate_async(self.batch._ptr, h))

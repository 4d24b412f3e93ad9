"""BatchLinearization: the discrete-time linearisation of the step for a whole batch,

    x' ~ A dx + B du,    y ~ C dx + D du,

by finite differences on the device -- mujoco's `mjd_transitionFD` for every environment at once.  What iLQR, MPC, LQR
stabilisers and system identification ask for next to `jacobian.BatchJacobian` and `dynamics.BatchDynamics`.

The reference asks one environment per call on the host and steps it once per column.  Here every perturbed copy of every
environment -- its columns -- is one environment of a second, scratch batch, and all of them are stepped by ONE launch of
the unchanged step kernel: a transition is three launches (fan-out, step, difference), whatever the model's size.

Conventions are MuJoCo's:
  * the state is x = [dq (nv), qvel (nv), act (na)], nx = 2 nv + na; A (B, nx, nx), B (B, nx, nu), C (B, nsensordata, nx),
    D (B, nsensordata, nu), row-major, A[e, i, j] = d x'_i / d x_j;
  * position columns are nudged with mj_integratePos along unit tangent j (ball and free rotations compose on the right),
    position rows are differenced with mj_differentiatePos;
  * every column starts from the nominal qacc_warmstart, time, mocap poses, qfrc_applied and xfrc_applied;
  * a control nudge is used only if both ctrl and ctrl +- eps lie inside ctrlrange of a ctrllimited actuator: central where
    both nudges are valid, one-sided against the nominal next state where one is, a zero column where neither;
    centered=False uses the forward nudge, or the backward one where the forward one is out of range;
  * the transition is `nstep` plain mj_steps (nstep = n_sub_steps gives the control-step transition); C and D are the
    derivatives of the sensordata the last of them writes.  Every column takes a full step: there are no skip stages.

The source batch is read, never written: unlike mjd_transitionFD there is nothing to restore.

Precision.  The scratch batch is fp64 by default, also under an fp32 batch: a difference quotient at eps = 1e-6 is
meaningless in fp32.  The fp32 state is converted up in the fan-out, stepped by the fp64 kernels, and A .. D are converted
down on the store (the outputs are tensors in the SOURCE batch's real type).  precision=32 on an fp32 batch steps the
columns in fp32: it needs a large eps (2**-10 or so) and gives two to three digits; see README.  precision=32 on an fp64
batch is refused.

Model edits made to the source batch before this object was created (`set_model_real`, `set_opt`) are replayed on the
scratch batch from the source's host record; edits made afterwards need a new object, as with BatchDynamics.  Per-environment
geoms (`set_env_geoms`) are not mirrored: such a batch is refused.  A transition contains a step launch of another batch and
is not meant for HIP-graph capture.
"""
import ctypes

import numpy as np

from dm_control_amd import _native
from dm_control_amd import _unit
from dm_control_amd import batch as batch_lib

_JNT_NQ = (7, 4, 1, 1)
_JNT_NV = (6, 3, 1, 1)
_SKIP_OPTS = ('stash',)      # launch tuning of the source batch, not part of the model


class _Tables(ctypes.Structure):      # dmc_lin_tables
  _fields_ = [(n, ctypes.c_int32) for n in ('nj', 'nq', 'nv', 'na', 'nu', 'nints', 'nreals')] + \
             [('ints', ctypes.c_void_p), ('reals', ctypes.c_void_p)]


def model_tables(model, ctrlrange=None):
  """dict(dims, ints, reals) of a compiled model as dmc_lin_create takes them (include/dmc_lin.h): the joint table (type,
  qpos address, dof address per joint) and ctrllimited / ctrlrange per actuator (`ctrlrange`: the live values where the
  batch's were edited)."""
  m = model
  nj, nu = int(m.njnt), int(m.nu)
  cr = np.asarray(m.actuator_ctrlrange if ctrlrange is None else ctrlrange, dtype=np.float64).reshape(-1)
  if cr.size != 2 * nu:
    raise ValueError('linearize: ctrlrange holds %d values, 2 nu = %d expected' % (cr.size, 2 * nu))
  ints = np.concatenate([np.asarray(a, dtype=np.int32).reshape(-1) for a in
                         (m.jnt_type, m.jnt_qposadr, m.jnt_dofadr, m.actuator_ctrllimited)] + [np.zeros(0, np.int32)])
  dims = dict(nj=nj, nq=int(m.nq), nv=int(m.nv), na=int(m.na), nu=nu, nx=2 * int(m.nv) + int(m.na),
              nsensordata=int(m.nsensordata))
  return dict(dims=dims, ints=np.ascontiguousarray(ints, dtype=np.int32), reals=np.ascontiguousarray(cr))


def columns(nx, nu, centered=True):
  """P: the scratch environments one linearised environment takes (csrc/lin_core.h lin_ncol)."""
  return 1 + (nx + nu) + ((nx + nu) if centered else nu)


def chunk_envs(batch_size, P, max_scratch_envs):
  """Source environments per chunk: all of them where B P fits `max_scratch_envs`, else max_scratch_envs // P."""
  if P > max_scratch_envs:
    raise ValueError('linearize: one environment needs %d scratch environments, max_scratch_envs = %d' % (P, max_scratch_envs))
  return min(int(batch_size), int(max_scratch_envs) // P)


class BatchLinearization(_unit.BatchUnit):
  """A, B (and C, D) of mjd_transitionFD for every environment of a batch; see the module docstring.

  physics: a `BatchedPhysics`, or anything holding one as `.batch` (Physics) or `.physics`.
  eps: the nudge (> 0).  centered: central differences (2 (nx + nu) + 1 columns per environment) or forward ones
  (nx + 2 nu + 1).  nstep: mj_steps per transition.  precision: of the scratch batch, 64 (default) or 32.
  max_scratch_envs: the scratch batch holds at most this many environments; a larger B P is linearised in chunks on the
  one stream.  nconmax / njmax / njcon: the scratch batch's capacities (default: what the source batch was created with).
  The model's tables and the source batch's recorded model edits are read here; edits made afterwards need a new object.
  """
  _DESTROY = 'dmc_lin_destroy'
  _OUT_ERROR = 'out: expected contiguous %s tensors, this one of shape %s, on %s'

  def __init__(self, physics, eps=1e-6, centered=True, nstep=1, precision=64, max_scratch_envs=1 << 16,
               nconmax=None, njmax=None, njcon=None):
    batch = _unit.find_batch(physics)
    if batch is None:
      raise ValueError('linearize: no batch inside %r (a BatchedPhysics, or an object holding one as .batch / .physics, is needed)'
                       % (type(physics).__name__,))
    if getattr(batch, 'env_geoms', None):
      raise ValueError('linearize: the batch declares per-environment geoms %s, which are not mirrored to the scratch batch'
                       % (list(batch.env_geoms),))
    if not (isinstance(eps, (int, float, np.floating, np.integer)) and np.isfinite(eps) and eps > 0):
      raise ValueError('linearize: eps must be a positive number, got %r' % (eps,))
    if int(nstep) < 1:
      raise ValueError('linearize: nstep must be >= 1, got %r' % (nstep,))
    if int(precision) not in (32, 64):
      raise ValueError('linearize: precision must be 32 or 64, got %r' % (precision,))
    if int(precision) < int(batch.precision):
      raise ValueError('linearize: precision=32 cannot linearise an fp64 batch (the scratch batch is never less precise than the source)')
    self.batch, self.model = batch, batch.model
    self.tables = model_tables(self.model, batch.model_real.get('actuator_ctrlrange'))
    d = self.tables['dims']
    self.nx, self.nu, self.nsensordata = d['nx'], d['nu'], d['nsensordata']
    if self.nx == 0:
      raise ValueError('linearize: the model has no state (nx = 2 nv + na = 0)')
    self.eps, self.centered, self.nstep, self.precision = float(eps), bool(centered), int(nstep), int(precision)
    self.P = columns(self.nx, self.nu, self.centered)
    self.chunk = chunk_envs(batch.batch_size, self.P, int(max_scratch_envs))
    caps = tuple(getattr(batch, '_user_caps', (0, 0, 0)))
    caps = tuple(int(c if v is None else v) for c, v in zip(caps, (nconmax, njmax, njcon)))
    self._ptr = ctypes.c_void_p()
    self.scratch = batch_lib.BatchedPhysics(self.model, self.chunk * self.P, device_id=batch.device_id, precision=self.precision,
                                            nconmax=caps[0], njmax=caps[1], njcon=caps[2])
    self.scratch.legacy_step = False
    for name, values in batch.model_real.items():
      self.scratch.set_model_real(name, values)
    for name, value in getattr(batch, 'opts', {}).items():
      if name not in _SKIP_OPTS:
        self.scratch.set_opt(name, value)
    self.scratch.set_output_mask(0)      # the state is all a transition without sensors reads
    tb = _Tables(d['nj'], d['nq'], d['nv'], d['na'], d['nu'], self.tables['ints'].size, self.tables['reals'].size,
                 self.tables['ints'].ctypes.data, self.tables['reals'].ctypes.data)
    _native.check(_native.lib().dmc_lin_create(batch._ptr, self.scratch._ptr, ctypes.byref(tb), self.eps, int(self.centered),
                                                self.nstep, ctypes.byref(self._ptr)))

  def close(self):
    super().close()
    if getattr(self, 'scratch', None) is not None:
      self.scratch.close()
      self.scratch = None

  def info(self):
    a = np.zeros(12, dtype=np.int32)
    _native.check(_native.lib().dmc_lin_info(self._ptr, a.ctypes.data))
    out = dict(zip(('B', 'columns', 'nx', 'nu', 'nsensordata', 'scratch_envs', 'chunk', 'precision', 'scratch_precision', 'nstep',
                    'centered', 'block'), (int(x) for x in a)))
    out['chunks'] = -(-out['B'] // out['chunk'])
    return out

  def transition(self, sensors=False, out=None, stream=None):
    """(A, B), or (A, B, C, D) with sensors=True, at the state the batch holds; tensors in the batch's real type on its
    device.  `out`: a tuple of tensors to write in place (every element is written).  Asynchronous on `stream` (a torch
    stream or a raw handle; default: torch's current stream): per chunk of environments a fan-out, a step launch of the
    scratch batch and a difference.  The batch itself is not written; the host is never read."""
    _, _, dt = self._torch()
    B, nx, nu, ns = self.batch.batch_size, self.nx, self.nu, self.nsensordata
    shapes = [(B, nx, nx), (B, nx, nu)] + ([(B, ns, nx), (B, ns, nu)] if sensors else [])
    if out is not None and len(out) != len(shapes):
      raise ValueError('out: expected %d tensors, got %d' % (len(shapes), len(out)))
    res = [self._tensor(s, dt, None if out is None else out[k]) for k, s in enumerate(shapes)]
    mask = batch_lib.OUT['sensor'] if sensors else 0
    if self.scratch.output_mask != mask:
      self.scratch.set_output_mask(mask)
    self.scratch._poll_specialised()      # pylint: disable=protected-access  (a kernel built in the background takes over here)
    h = self.stream_handle(stream)
    ptr = [t.data_ptr() if t.numel() else None for t in res] + [None, None]      # (an empty tensor, nu = 0: no pointer)
    L = _native.lib()
    for first in range(0, B, self.chunk):
      _native.check(L.dmc_lin_transition(self._ptr, first, min(self.chunk, B - first), ptr[0], ptr[1], ptr[2], ptr[3], h))
    return tuple(res)

  def fan_out(self, first_env=0, stream=None):
    """The first launch of a transition alone: the perturbed columns of the chunk that starts at `first_env` are written to
    `self.scratch` (environment e of the chunk, column c: scratch environment e P + c) and nothing is stepped.  For
    inspection; returns the number of source environments fanned out."""
    n = min(self.chunk, self.batch.batch_size - int(first_env))
    _native.check(_native.lib().dmc_lin_fan_out(self._ptr, int(first_env), n, self.stream_handle(stream)))
    return n

  def warnings(self, stream=None):
    """(B,) int32: bit w set where some column of the environment raised warning w (mjtWarning order) in the last
    transition -- e.g. bit 1, mjWARN_CONTACTFULL, where a perturbed copy ran out of contact slots."""
    torch, dev, _ = self._torch()
    res = torch.empty((self.batch.batch_size,), dtype=torch.int32, device=dev)
    _native.check(_native.lib().dmc_lin_warnings(self._ptr, res.data_ptr(), self.stream_handle(stream)))
    return res

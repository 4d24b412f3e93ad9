"""TEST INFRASTRUCTURE: a plain numpy mjd_transitionFD, the reference of the linearisation unit's tests.

One column at a time: a fresh `oracle.OraclePhysics(legacy_step=False)` gets the perturbed state and takes `nstep` mj_steps;
the tangent space is `host_data.integrate_pos` / `differentiate_pos`.  Nothing here is the code under test: not the host
build of csrc/lin_core.h, not the device kernels, not the host seam.

Columns are numbered as the C ABI numbers them (include/dmc_lin.h), so that the stepped columns of the twin can be handed
to the host build of the difference: 0 the nominal state, 1 + j input j nudged up, then the nudged-down ones -- every input
when centred, the controls only otherwise.
"""
import numpy as np

from dm_control_amd import host_data
from oracle.oracle import OracleModel, OraclePhysics

STATE = ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart', 'qfrc_applied')
FWD, BACK = 1, 2


def oracle_model(model, model_real=None, opts=None):
  """The oracle's model with the batch-wide edits a test made (`set_model_real`, `set_opt`) applied."""
  om = OracleModel(model)
  for name, values in (model_real or {}).items():
    om.field(name)[:] = np.asarray(values, dtype=np.float64).ravel()
  for name, value in (opts or {}).items():
    if isinstance(value, (int, np.integer)):
      om.opt_int(name, int(value))
    else:
      om.opt_real(name, float(value))
  return om


def in_range(x1, x2, lo, hi):
  return lo <= x1 <= hi and lo <= x2 <= hi


def ctrl_flags(model, ctrl, eps, centered, ctrlrange=None):
  """mjd_transitionFD's rule per control: FWD | BACK, the nudges that are taken."""
  cr = np.asarray(model.actuator_ctrlrange if ctrlrange is None else ctrlrange, dtype=np.float64).reshape(-1, 2)
  out = []
  for k in range(model.nu):
    limited = bool(model.actuator_ctrllimited[k])
    u = float(ctrl[k])
    fwd = (not limited) or in_range(u, u + eps, cr[k, 0], cr[k, 1])
    back = (centered or not fwd) and ((not limited) or in_range(u - eps, u, cr[k, 0], cr[k, 1]))
    out.append((FWD if fwd else 0) | (BACK if back else 0))
  return np.array(out, dtype=np.int32)


def column_inputs(model, centered):
  """[(input index or -1, sign)] per column."""
  nx, nu = 2 * model.nv + model.na, model.nu
  n = nx + nu
  cols = [(-1, 0)] + [(j, 1) for j in range(n)]
  cols += [(j, -1) for j in (range(n) if centered else range(nx, n))]
  return cols


def perturbed(model, state, eps, centered=True, ctrlrange=None):
  """The P perturbed copies of `state` ({qpos, qvel, act, ctrl, ...: arrays}) and the control flags."""
  m, nv, na = model, model.nv, model.na
  nx = 2 * nv + na
  flags = ctrl_flags(m, state['ctrl'], eps, centered, ctrlrange)
  out = []
  for j, sign in column_inputs(m, centered):
    s = {k: np.array(v, dtype=np.float64).ravel().copy() for k, v in state.items()}
    h = sign * eps
    if 0 <= j < nv:
      dq = np.zeros(nv)
      dq[j] = 1.0
      host_data.integrate_pos(m, s['qpos'], dq, h)
    elif nv <= j < 2 * nv:
      s['qvel'][j - nv] += h
    elif 2 * nv <= j < nx:
      s['act'][j - 2 * nv] += h
    elif j >= nx and flags[j - nx] & (FWD if sign > 0 else BACK):
      s['ctrl'][j - nx] += h
    out.append(s)
  return out, flags


def step_column(om, s, nstep):
  """A fresh environment at state `s`, stepped: dict(qpos, qvel, act, sensordata, ncon, warning)."""
  p = OraclePhysics(om, legacy_step=False)
  for k in STATE:
    if k in s and np.size(s[k]):
      p.field(k)[:] = np.asarray(s[k], dtype=np.float64).ravel()
  p.time = float(np.ravel(s.get('time', 0.0))[0])
  p.step(int(nstep))
  g = lambda n: np.array(p.field(n), dtype=np.float64).ravel().copy()
  return dict(qpos=g('qpos'), qvel=g('qvel'), act=g('act') if om.compiled.na else np.zeros(0),
              sensordata=g('sensordata') if om.compiled.nsensordata else np.zeros(0), ncon=int(p.ncon), warning=np.array(p.warning).copy())


def difference(model, stepped, flags, eps, centered=True):
  """A, B, C, D from the stepped columns ([dict(qpos, qvel, act, sensordata)] in column order)."""
  m, nv, na, nu, ns = model, model.nv, model.na, model.nu, model.nsensordata
  nx = 2 * nv + na
  n = nx + nu
  AB, CD = np.zeros((nx, n)), np.zeros((ns, n))
  for j in range(n):
    f = (FWD | (BACK if centered else 0)) if j < nx else int(flags[j - nx])
    if not f:
      continue
    minus = 1 + n + (j if centered else j - nx)
    a = stepped[1 + j] if f & FWD else stepped[0]
    b = stepped[minus] if f & BACK else stepped[0]
    h = 2 * eps if f == (FWD | BACK) else eps
    dq = np.zeros(nv)
    host_data.differentiate_pos(m, dq, h, b['qpos'], a['qpos'])
    AB[:nv, j] = dq
    AB[nv:2 * nv, j] = (a['qvel'] - b['qvel']) / h
    AB[2 * nv:, j] = (a['act'] - b['act']) / h
    CD[:, j] = (a['sensordata'] - b['sensordata']) / h
  return AB[:, :nx].copy(), AB[:, nx:].copy(), CD[:, :nx].copy(), CD[:, nx:].copy()


def transition_fd(model, state, eps=1e-6, centered=True, nstep=1, model_real=None, opts=None):
  """dict(A, B, C, D, flags, columns (the perturbed states), stepped, ncon (per column)) at `state`."""
  cr = (model_real or {}).get('actuator_ctrlrange')
  om = oracle_model(model, model_real, opts)
  cols, flags = perturbed(model, state, eps, centered, cr)
  stepped = [step_column(om, s, nstep) for s in cols]
  A, B, C, D = difference(model, stepped, flags, eps, centered)
  return dict(A=A, B=B, C=C, D=D, flags=flags, columns=cols, stepped=stepped, ncon=np.array([s['ncon'] for s in stepped]))


def stack(cols, fields):
  """{field: (P, rows)} of a list of per-column dicts."""
  return {f: np.stack([np.asarray(c[f], dtype=np.float64).ravel() for c in cols]) for f in fields}

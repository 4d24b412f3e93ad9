"""Batched linearisation without a GPU: the host build of csrc/lin_core.h (tests/emu/lin_emu.cpp) in both scratch real types
against the numpy twin (tests/lin_twin.py: mjd_transitionFD column by column on the fp64 oracle) -- the fan-out, the
validity flags of clamped controls, the difference fed the twin's own stepped columns, the whole pipeline on every model
and state, the closed form of the linear model, the host seam's mjd_transitionFD, the refusals, the C entry points'
argument checks, and a sanitized stand-alone program."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lin_emu_lib as emu      # noqa: E402
import lin_twin as tw      # noqa: E402
import linearize_cases as lc      # noqa: E402
from dm_control_amd import host_data      # noqa: E402
from dm_control_amd import linearize      # noqa: E402

STEPPED = ('qpos', 'qvel', 'act', 'sensordata')
INPUTS = ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart', 'qfrc_applied')
ULP = np.finfo(np.float64).eps


@pytest.fixture(scope='module')
def world():
  """Per model: the compiled model, its tables, its states and the twin's result at every state (centred, EPS)."""
  w = {}
  for name in lc.MODELS:
    m = lc.model(name)
    st = lc.states(name)
    w[name] = dict(m=m, tables=linearize.model_tables(m), states=st, ref=[tw.transition_fd(m, s, lc.EPS, True) for s in st])
  return w


def quats(m):
  """qpos addresses of the quaternions."""
  return [int(a) + (3 if int(t) == 0 else 0) for t, a in zip(m.jnt_type, m.jnt_qposadr) if int(t) < 2]


def host_pipeline(prec, m, tables, state, eps, centered=True, nstep=1, stepper=None):
  """Host fan-out, one step per column (the fp64 oracle, or `stepper`), host difference."""
  cols, flags = emu.fan(prec, m, tables, eps, state, centered)
  om = tw.oracle_model(m)
  step = stepper or (lambda s: tw.step_column(om, s, nstep))
  stepped = [step({k: cols[k][c] for k in cols}) for c in range(cols['qpos'].shape[0])]
  return emu.diff(prec, m, tables, eps, tw.stack(stepped, STEPPED), flags, centered)


def test_states_are_as_recorded(world):
  for name in lc.MODELS:
    assert tuple(s['ncon'] for s in world[name]['states']) == lc.NCON[name], name
    for s, ref in zip(world[name]['states'], world[name]['ref']):
      assert set(ref['ncon'].tolist()) == {int(ref['ncon'][0])}, (name, 'a column changed its contact count at eps = 1e-6')
      assert not any(c['warning'].any() for c in ref['stepped'])
  m = world['leg']['m']
  assert (m.nq, m.nv, m.na, m.nu, m.nsensordata) == (13, 11, 1, 3, 8)
  assert linearize.columns(2 * 9, 6) == 49 and linearize.columns(2 * 27, 21) == 151 and linearize.columns(23, 3) == 53
  assert linearize.columns(23, 3, centered=False) == 1 + 23 + 2 * 3


@pytest.mark.parametrize('centered', [True, False])
def test_fan_out_against_the_twin(world, centered):
  rs = np.random.RandomState(5)
  for name in ('leg', 'humanoid', 'cheetah'):
    w = world[name]
    m, tb = w['m'], w['tables']
    for s in w['states']:
      s = dict(s, qfrc_applied=rs.uniform(-1, 1, m.nv), xfrc_applied=rs.uniform(-1, 1, 6 * m.nbody))
      want, wflags = tw.perturbed(m, {k: s[k] for k in INPUTS}, lc.EPS, centered)
      want = tw.stack(want, INPUTS)
      cols, flags = emu.fan(64, m, tb, lc.EPS, s, centered, xfrc=True)
      P = linearize.columns(2 * m.nv + m.na, m.nu, centered)
      assert cols['qpos'].shape == (P, m.nq) and np.array_equal(flags, wflags)
      for k in INPUTS:
        assert np.abs(cols[k] - want[k]).max(initial=0) <= 1e-14 * max(1.0, np.abs(want[k]).max(initial=0)), (name, k)
      for a in quats(m):
        assert np.abs(np.sqrt((cols['qpos'][:, a:a + 4] ** 2).sum(axis=1)) - 1).max() <= 4 * ULP, (name, a)
      # what a column does not nudge is a copy, bit for bit: the whole nominal column, the warm start, the applied forces,
      # the time, and every entry of qpos / qvel / act / ctrl outside the nudged joint
      for k in INPUTS + ('xfrc_applied', 'time'):
        assert np.array_equal(cols[k][0], np.asarray(s[k], dtype=np.float64).ravel()), (name, k)
      for k in ('qacc_warmstart', 'qfrc_applied', 'xfrc_applied', 'time'):
        assert np.array_equal(cols[k], np.broadcast_to(cols[k][0], cols[k].shape)), (name, k)
      for c, (j, sign) in enumerate(tw.column_inputs(m, centered)):
        changed = {k: np.nonzero(cols[k][c] != cols[k][0])[0] for k in ('qpos', 'qvel', 'act', 'ctrl')}
        nv, nx = m.nv, 2 * m.nv + m.na
        where = 'qpos' if 0 <= j < nv else 'qvel' if j < 2 * nv else 'act' if j < nx else 'ctrl'
        for k, idx in changed.items():
          if j < 0 or k != where:
            assert idx.size == 0, (name, c, k)
          elif k == 'ctrl':      # (a nudge the clamped rule does not take leaves the nominal control)
            assert idx.tolist() == ([j - nx] if flags[j - nx] & (tw.FWD if sign > 0 else tw.BACK) else []), (name, c)
          elif k != 'qpos':
            assert idx.tolist() == [j - dict(qvel=nv, act=2 * nv)[k]], (name, c, k)
          else:
            jn = max(i for i in range(m.njnt) if int(m.jnt_dofadr[i]) <= j)
            a0 = int(m.jnt_qposadr[jn])
            assert idx.size and idx.min() >= a0 and idx.max() < a0 + host_data.JNT_NQ[int(m.jnt_type[jn])], (name, c)
      # the fp32 scratch type: every column holds fp32 values, the copies are exact
      s32 = {k: np.asarray(v, dtype=np.float32).astype(np.float64) for k, v in s.items() if k not in ('ncon', 'time')}
      c32, _ = emu.fan(32, m, tb, lc.EPS32, dict(s32, time=s['time']), centered, xfrc=True)
      for k in INPUTS + ('xfrc_applied',):
        assert np.array_equal(c32[k], c32[k].astype(np.float32).astype(np.float64)) and np.array_equal(c32[k][0], s32[k].ravel())
      w32, _ = tw.perturbed(m, {k: s32[k] for k in INPUTS}, lc.EPS32, centered)
      w32 = tw.stack(w32, INPUTS)
      assert max(np.abs(c32[k] - w32[k]).max(initial=0) for k in INPUTS) <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(w32['qpos']).max())


def test_validity_flags_of_clamped_controls(world):
  """leg: a ctrllimited motor in [-1, 1], an unlimited filter actuator, a ctrllimited servo in [-0.05, 0.05]."""
  w = world['leg']
  m, tb, s0 = w['m'], w['tables'], w['states'][0]
  F, Bk = tw.FWD, tw.BACK
  cases = [  # ctrl, flags centred, flags forward
      ((1.0, 7.0, -0.05), (Bk, F | Bk, F), (Bk, F, F)),              # at the upper limit, unlimited, at the lower limit
      ((0.2, -3.0, 0.01), (F | Bk,) * 3, (F,) * 3),                   # strictly inside
      ((1.0 - lc.EPS / 2, 0.0, -0.05 + lc.EPS / 2), (Bk, F | Bk, F), (Bk, F, F)),      # closer to a limit than eps
      ((1.5, 0.0, -0.2), (0, F | Bk, 0), (0, F, 0)),                  # outside the range: no nudge is valid
  ]
  nx = 2 * m.nv + m.na
  for ctrl, centred_flags, forward_flags in cases:
    for centered, want in ((True, centred_flags), (False, forward_flags)):
      s = dict(s0, ctrl=np.array(ctrl))
      assert tuple(tw.ctrl_flags(m, s['ctrl'], lc.EPS, centered)) == want
      # fp32 columns: the control the column holds (-0.05f lies outside [-0.05, 0.05]) against the fp64 range, as the twin
      # judges that value
      c32 = np.asarray(ctrl, dtype=np.float32).astype(np.float64)
      _, f32 = emu.fan(32, m, tb, lc.EPS32, dict(s0, ctrl=c32), centered)
      assert tuple(f32) == tuple(tw.ctrl_flags(m, c32, lc.EPS32, centered)), (ctrl, centered)
      if ctrl[2] == -0.05:
        assert f32[2] == 0 and f32[0] == want[0]      # (1.0f is 1.0: still at the limit)
      cols, flags = emu.fan(64, m, tb, lc.EPS, s, centered)
      n = nx + m.nu
      for k in range(m.nu):
        up, dn = cols['ctrl'][1 + nx + k, k], cols['ctrl'][1 + n + (nx + k if centered else k), k]
        assert up == (ctrl[k] + lc.EPS if want[k] & F else ctrl[k]) and dn == (ctrl[k] - lc.EPS if want[k] & Bk else ctrl[k])
      # ... and the columns of A .. D follow them: central, one-sided against the nominal column, or zero
      ref = tw.transition_fd(m, s, lc.EPS, centered)
      A, B, C, D = emu.diff(64, m, tb, lc.EPS, tw.stack(ref['stepped'], STEPPED), flags, centered)
      assert np.array_equal(B[m.nv:], ref['B'][m.nv:]) and np.array_equal(D, ref['D'])
      assert lc.rel_err(B, ref['B']) <= lc.F64_TOL
      st = ref['stepped']
      for k in range(m.nu):
        if want[k] == 0:
          assert not B[:, k].any() and not D[:, k].any()
        elif want[k] == Bk:
          minus = st[1 + n + (nx + k if centered else k)]
          assert np.array_equal(B[m.nv:2 * m.nv, k], (st[0]['qvel'] - minus['qvel']) / lc.EPS) and B[:, k].any()
        elif want[k] == F:
          assert np.array_equal(B[m.nv:2 * m.nv, k], (st[1 + nx + k]['qvel'] - st[0]['qvel']) / lc.EPS)


@pytest.mark.parametrize('centered', [True, False])
def test_difference_of_the_twins_stepped_columns(world, centered):
  for name in lc.MODELS:
    w = world[name]
    m, tb = w['m'], w['tables']
    nv = m.nv
    for i, s in enumerate(w['states']):
      ref = w['ref'][i] if centered else tw.transition_fd(m, s, lc.EPS, False)
      A, B, C, D = emu.diff(64, m, tb, lc.EPS, tw.stack(ref['stepped'], STEPPED), ref['flags'], centered)
      assert not any(np.isnan(x).any() for x in (A, B, C, D))      # every element is written
      # velocity, activation and sensor rows: the same quotient, the same bits
      assert np.array_equal(A[nv:], ref['A'][nv:]) and np.array_equal(B[nv:], ref['B'][nv:]), (name, i)
      assert np.array_equal(C, ref['C']) and np.array_equal(D, ref['D']), (name, i)
      # position rows: mju_subQuat with the header's own arc tangent
      assert lc.rel_err(A[:nv], ref['A'][:nv]) <= lc.F64_TOL and lc.rel_err(B[:nv], ref['B'][:nv]) <= lc.F64_TOL, (name, i)
      g = emu.diff(64, m, tb, lc.EPS, tw.stack(ref['stepped'], STEPPED), ref['flags'], centered, sensors=False)
      assert np.array_equal(g[0], A) and np.array_equal(g[1], B) and np.isnan(g[2]).all() and np.isnan(g[3]).all()


def test_sub_quat_against_numpy():
  """The header's arc tangent over every octant and magnitude, against host_data's mju_subQuat (numpy.arctan2)."""
  rs = np.random.RandomState(11)
  worst = 0.0
  for ang in (0.0, 1e-12, 1e-6, 1e-3, 0.3, 0.7, 0.8, 1.5, 1.6, 2.4, 3.0, np.pi - 1e-9, np.pi, np.pi + 1e-9, 4.0, 6.0):
    for _ in range(8):
      ax = rs.normal(size=3)
      ax /= np.linalg.norm(ax)
      qb = rs.normal(size=4)
      qb /= np.linalg.norm(qb)
      qa = host_data.quat_mul_rows(qb, np.concatenate([[np.cos(ang / 2)], ax * np.sin(ang / 2)]))
      want = host_data._quat_sub(qa, qb)      # pylint: disable=protected-access
      got = emu.sub_quat(64, qa, qb)
      if abs(abs(ang) - np.pi) > 1e-6:      # (at a half turn the sign of the rotation vector is a coin toss of the last bit)
        worst = max(worst, np.abs(got - want).max())
        assert np.abs(got - want).max() <= 1e-14 * max(1.0, ang), (ang, got, want)
      else:
        assert abs(np.linalg.norm(got) - np.linalg.norm(want)) <= 1e-14 * np.pi
      g32 = emu.sub_quat(32, qa, qb)
      if abs(abs(ang) - np.pi) > 1e-3:
        assert np.abs(g32 - want).max() <= 2e-6 * max(1.0, ang), (ang, g32, want)
  print('sub_quat: worst |host build - numpy| = %.3g' % worst)


def test_pipeline_on_every_model_and_state(world):
  """Host fan-out, the oracle's mj_step per column, host difference, against the twin at equal eps."""
  measured = {}
  for name in lc.MODELS:
    w = world[name]
    m, tb = w['m'], w['tables']
    for i, s in enumerate(w['states']):
      for centered, nstep in ((True, 1), (False, 1), (True, 3)):
        ref = w['ref'][i] if (centered and nstep == 1) else tw.transition_fd(m, s, lc.EPS, centered, nstep)
        got = host_pipeline(64, m, tb, s, lc.EPS, centered, nstep)
        err = lc.worst(got, ref)
        kind = 'contact' if s['ncon'] else 'free'
        measured[(name, kind)] = max(measured.get((name, kind), 0.0), err)
        bound = lc.F64_TOL if not s['ncon'] else 4 * lc.PIPELINE_F64_MEASURED[name]
        assert err <= bound, (name, i, centered, nstep, err, bound)
  for k in sorted(measured):
    print('fp64 host pipeline against the twin, %s, %s states: worst error / max(1, |ref|max) = %.3g' % (k + (measured[k],)))


def emu_stepper(m, prec, time):
  """One step of a column on the host build of the step core in `prec` (tests/emu_lib.py): the fp32 CPU stepper."""
  import emu_lib      # pylint: disable=import-outside-toplevel

  def step(s):
    p = emu_lib.EmuPhysics(m, prec=prec)
    for k in ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart', 'qfrc_applied'):
      if np.size(s[k]):
        getattr(p, k)[:] = s[k]
    p.time[:] = time
    p.step(1, legacy=False)
    return {k: np.array(getattr(p, k), dtype=np.float64).copy() for k in STEPPED}
  return step


def test_fp32_pipeline_measures_what_the_fp32_scratch_mode_gives(world):
  """Fan-out, step (the host build of the step core) and difference all in fp32 at eps = 2**-10, against the fp64 twin at
  the fp32 state and the same eps: the accuracy of precision=32, and the base of the GPU tier's bound for it."""
  for name in ('leg', 'cheetah'):
    w = world[name]
    m, tb = w['m'], w['tables']
    worst = 0.0
    for s in lc.env_states(name):      # (the environments of the GPU tier's batch, the clamped controls among them)
      s32 = {k: np.asarray(v, dtype=np.float32).astype(np.float64) for k, v in s.items() if k not in ('ncon', 'time')}
      s32['time'] = s['time']
      ref = tw.transition_fd(m, s32, lc.EPS32, True)
      got = host_pipeline(32, m, tb, s32, lc.EPS32, True, stepper=emu_stepper(m, 32, s['time']))
      worst = max(worst, lc.worst(got, ref))
    print('fp32 host pipeline against the fp64 twin at eps = 2**-10, %s: worst error / max(1, |ref|max) = %.3g' % (name, worst))
    assert worst <= 4 * lc.PIPELINE_F32_MEASURED[name], (name, worst)


def test_closed_form_of_the_linear_model(world):
  """lqr_2_1: slides, springs and dampers.  v' = v + h (M + h D)^-1 (-K q - D v + G u), q' = q + h v'."""
  from oracle.oracle import OraclePhysics
  w = world['lqr_2_1']
  m, tb = w['m'], w['tables']
  assert all(int(t) == 2 for t in m.jnt_type) and m.na == 0
  nv, nu, h = m.nv, m.nu, float(m.opt.timestep)
  p = OraclePhysics(m, legacy_step=False)
  p.forward()
  M = np.asarray(p.qM, dtype=np.float64).reshape(nv, nv)
  K, Dm = np.diag(np.asarray(m.jnt_stiffness, dtype=np.float64)), np.diag(np.asarray(m.dof_damping, dtype=np.float64))
  G = np.zeros((nv, nu))
  for k in range(nu):
    G[int(m.actuator_trnid[2 * k]) if np.ndim(m.actuator_trnid) == 1 else int(m.actuator_trnid[k][0]), k] = \
        float(np.asarray(m.actuator_gear).reshape(nu, 6)[k, 0]) * float(np.asarray(m.actuator_gainprm).reshape(nu, -1)[k, 0])
  eulerdamp_off = bool(int(m.opt.disableflags) & host_data.C.get('DMC_DSBL_EULERDAMP', 0))
  Minv = np.linalg.inv(M if eulerdamp_off else M + h * Dm)
  Avq, Avv, Bv = -h * Minv @ K, np.eye(nv) - h * Minv @ Dm, h * Minv @ G
  A_ref = np.block([[np.eye(nv) + h * Avq, h * Avv], [Avq, Avv]])
  B_ref = np.vstack([h * Bv, Bv])
  results = []
  for s in w['states']:
    for eps in (1e-6, 1e-4):
      A, B, _, _ = host_pipeline(64, m, tb, s, eps)
      assert lc.rel_err(A, A_ref) <= lc.F64_TOL and lc.rel_err(B, B_ref) <= lc.F64_TOL, (eps, lc.rel_err(A, A_ref), lc.rel_err(B, B_ref))
      results.append(A)
  for A in results[1:]:      # a linear system: the same A at every state and every eps
    assert lc.rel_err(A, results[0]) <= lc.F64_TOL


def test_host_seam_mjd_transition_fd(world, monkeypatch):
  import oracle_backend as ob
  from dm_control_amd import mujoco_api as mj
  monkeypatch.setattr(mj, 'BatchedPhysics', ob.OracleBatch)
  w = world['leg']
  m = w['m']
  nx, nu, ns = 2 * m.nv + m.na, m.nu, m.nsensordata
  mm = mj.MjModel.from_xml_string(lc.LEG_XML)
  for i, ctrl in ((0, None), (2, (1.0, 0.3, -0.05))):
    s = dict(w['states'][i])
    if ctrl is not None:
      s['ctrl'] = np.array(ctrl)
    dd = mj.MjData(mm)
    for k in ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart'):
      getattr(dd, k)[:] = s[k]
    dd.time = float(s['time'][0])
    for centered in (True, False):
      before = {k: np.array(getattr(dd, k)).copy() for k in ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart')}
      A, B, C, D = np.full((nx, nx), np.nan), np.full((nx, nu), np.nan), np.full((ns, nx), np.nan), np.full((ns, nu), np.nan)
      mj.mjd_transitionFD(mm, dd, lc.EPS, centered, A, B, C, D)
      ref = tw.transition_fd(m, s, lc.EPS, centered)
      assert lc.worst((A, B, C, D), ref) <= lc.F64_TOL, (i, centered, lc.worst((A, B, C, D), ref))
      for k, v in before.items():      # d is as it was found, in every bit
        assert np.array_equal(np.asarray(getattr(dd, k)), v) and np.asarray(getattr(dd, k)).tobytes() == v.tobytes(), k
      assert dd.time == float(s['time'][0])
      mj.mjd_transitionFD(mm, dd, lc.EPS, centered, A, None, None, None)      # any output may be left out
  with pytest.raises(mj.FatalError, match='A must have'):
    mj.mjd_transitionFD(mm, dd, lc.EPS, True, np.zeros((nx, nx + 1)), None, None, None)
  with pytest.raises(mj.FatalError, match='eps'):
    mj.mjd_transitionFD(mm, dd, 0.0, True, None, None, None, None)


def test_refusals_are_loud(world):
  from dm_control_amd import mjcf_compiler as mc
  m = world['leg']['m']
  fake = lambda **kw: types.SimpleNamespace(**dict(dict(device_ptr=None, set_output_mask=None, model=m, model_real={}, opts={}, batch_size=4,
                                                        precision=64, device_id=0, _user_caps=(0, 0, 0)), **kw))
  with pytest.raises(ValueError, match='no batch inside'):
    linearize.BatchLinearization(object())
  with pytest.raises(ValueError, match='per-environment geoms'):
    linearize.BatchLinearization(fake(env_geoms=['floor']))
  for bad in (0, -1e-6, float('nan'), float('inf'), None, 'x'):
    with pytest.raises(ValueError, match='eps'):
      linearize.BatchLinearization(fake(), eps=bad)
  with pytest.raises(ValueError, match='nstep'):
    linearize.BatchLinearization(fake(), nstep=0)
  with pytest.raises(ValueError, match='precision must be'):
    linearize.BatchLinearization(fake(), precision=16)
  with pytest.raises(ValueError, match='cannot linearise an fp64 batch'):
    linearize.BatchLinearization(fake(), precision=32)
  still = mc.compile_xml('<mujoco><worldbody><body><geom size=".1"/></body></worldbody></mujoco>')
  with pytest.raises(ValueError, match='nx = 2 nv'):
    linearize.BatchLinearization(fake(model=still))
  with pytest.raises(ValueError, match='needs 53 scratch environments'):
    linearize.BatchLinearization(fake(), max_scratch_envs=52)
  assert linearize.chunk_envs(5, 53, 2 * 53 + 10) == 2 and linearize.chunk_envs(5, 53, 1 << 16) == 5
  with pytest.raises(ValueError, match='ctrlrange'):
    linearize.model_tables(m, np.zeros(4))


def test_native_entry_points_validate_without_a_device():
  from dm_control_amd import build
  build.build()
  from dm_control_amd import _native
  with open(os.path.join(ROOT, 'include', 'dmc_lin.h')) as f:
    declared = set(re.findall(r'\b(dmc_lin_[a-z0-9_]+)\s*\(', f.read()))
  assert declared == set(_native.LIN_EXPORTS)
  L = _native.lib()
  assert not [n for n in sorted(declared) if not hasattr(L, n)]
  out = ctypes.c_void_p()
  buf = (ctypes.c_double * 16)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  assert L.dmc_lin_create(None, p, p, 1e-6, 1, 1, ctypes.byref(out)) != 0 and b'null' in L.dmc_last_error() and not out.value
  assert L.dmc_lin_create(p, p, p, 1e-6, 1, 1, None) != 0 and b'null' in L.dmc_last_error()
  assert L.dmc_lin_transition(None, 0, 1, p, p, None, None, None) != 0 and b'null' in L.dmc_last_error()
  assert L.dmc_lin_warnings(None, p, None) != 0 and L.dmc_lin_info(None, p) != 0
  L.dmc_lin_destroy(None)
  units = {u[0]: u for u in build._UNITS}
  assert 'lin_core.h' in units['lin_kernels.hip'][2] and '-ffp-contract=off' in units['lin_kernels.hip'][1]
  d = emu.dims_array(lc.model('leg'))
  sz = emu.sizes(d)
  tb = linearize.model_tables(lc.model('leg'))
  assert (sz['P'], sz['nx'], sz['nin']) == (53, 23, 26) and (sz['nints'], sz['nreals']) == (tb['ints'].size, tb['reals'].size)
  assert sz['block'] == 256
  for src in ('lin_core.h', 'lin_kernels.hip'):
    with open(os.path.join(build.CSRC, src)) as f:
      text = re.sub(r'//[^\n]*', '', f.read())
    # plain arithmetic: no assembly, no LDS, no call into a math library that rounds differently on the host
    assert not re.search(r'\basm\b|__asm|__shared__|\bsin\(|\bcos\(|atan2?\(', text.replace('lin_atan2(', '').replace('lin_atan_small(', ''))


def test_sanitized_stand_alone_program_on_the_leg(tmp_path, world):
  """csrc/lin_core.h under AddressSanitizer and UBSan: a program with its own main (tests/emu/lin_sanitize.cpp) runs the
  fan-out and the difference of the leg in both real types, centred and forward -- never through Python, never on a GPU."""
  exe = str(tmp_path / 'lin_sanitize')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                         '-Wno-unknown-pragmas', '-o', exe, os.path.join(ROOT, 'tests', 'emu', 'lin_sanitize.cpp')])
  w = world['leg']
  m, tb = w['m'], w['tables']
  num = lambda a: ' '.join(repr(float(x)) for x in np.asarray(a).ravel())
  for i in (0, 3):
    s = w['states'][i]
    for centered in (1, 0):
      ref = w['ref'][i] if centered else tw.transition_fd(m, s, lc.EPS, False)
      d = emu.dims_array(m, centered)
      nominal = np.concatenate([np.asarray(s[k], dtype=np.float64).ravel() for k in ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart', 'qfrc_applied', 'time')])
      stepped = np.concatenate([tw.stack(ref['stepped'], STEPPED)[k] for k in STEPPED], axis=1)
      text = '\n'.join([' '.join(str(int(x)) for x in d), ' '.join(str(int(x)) for x in tb['ints']), num(tb['reals']), repr(lc.EPS),
                        num(nominal), num(stepped)]) + '\n'
      res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, check=False)
      assert res.returncode == 0, res.stderr[-2000:]
      rows = [np.array([float(x) for x in l.split()]) for l in res.stdout.strip().split('\n')]
      assert len(rows) == 4      # per real type: the fanned columns, then A B C D
      cols, flags = emu.fan(64, m, tb, lc.EPS, s, bool(centered))
      want = np.concatenate([cols[k] for k in emu.FAN_FIELDS], axis=1).ravel()
      np.testing.assert_array_equal(rows[0], np.concatenate([flags, want]))
      got = emu.diff(64, m, tb, lc.EPS, tw.stack(ref['stepped'], STEPPED), flags, bool(centered))
      np.testing.assert_array_equal(rows[1], np.concatenate([x.ravel() for x in got]))

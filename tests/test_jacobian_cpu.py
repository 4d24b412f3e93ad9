"""CPU tier of the batched Jacobians (dm_control_amd/jacobian.py, csrc/jac_core.h): the host build of the device header in
both real types against the fp64 twin (host_data.joint_frames + point_jacobian on the oracle's poses), against central
differences of the oracle's kinematics (independent of the twin), against host_data.object_velocity; the host seam's
mj_jacGeom / mj_jacBodyCom / mj_jacPointAxis / mj_applyFT; the refusals; the sanitizers on a stand-alone program."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import jac_emu_lib as emu      # noqa: E402
import jacobian_cases as jc      # noqa: E402
from dm_control_amd import host_data      # noqa: E402
from dm_control_amd import jacobian      # noqa: E402

TARGETS = jc.MORE_TARGETS
T = len(TARGETS)


@pytest.fixture(scope='module')
def world():
  """The oracle's fp64 kinematics of every state, computed once: dict(m, qpos, qvel, and per state every mjData array
  the tests read)."""
  import oracle_backend as ob
  from dm_control_amd import physics as physics_lib
  saved = physics_lib.BatchedPhysics
  physics_lib.BatchedPhysics = ob.OracleBatch
  try:
    p = physics_lib.Physics.from_xml_string(jc.xml())
    m = p.model
    qpos, qvel = jc.states(m)
    fields = ('xpos', 'xquat', 'xmat', 'xipos', 'site_xpos', 'site_xmat', 'geom_xpos', 'geom_xmat', 'cvel', 'subtree_com')

    def forward(q, v=None):
      p.data.qpos[:] = q
      p.data.qvel[:] = 0 if v is None else v
      p.forward()
      return {f: np.array(p.batch.get(f), dtype=np.float64).reshape(-1) for f in fields}
    w = dict(m=m, qpos=qpos, qvel=qvel, forward=forward, data=[forward(q, v) for q, v in zip(qpos, qvel)])
    yield w
  finally:
    physics_lib.BatchedPhysics = saved


def _points(seed):
  return np.random.RandomState(seed).uniform(-2, 2, (T, 3))


def _wrench(seed):
  rs = np.random.RandomState(100 + seed)
  return rs.uniform(-1, 1, (T, 3)), rs.uniform(-1, 1, (T, 3))


def test_model_exercises_every_path():
  m = jc.model()
  assert m.nv == 74 and m.nv > 64
  types = [int(t) for t in m.jnt_type]
  assert {0, 1, 2, 3} <= set(types)
  b = m.name2id('slider', 'body')
  assert int(m.body_jntnum[b]) == 2 and float(m.qpos0[m.jnt_qposadr[m.name2id('slide', 'joint')]]) == 0.1
  assert abs(float(m.qpos0[m.jnt_qposadr[m.name2id('twist', 'joint')]]) - np.deg2rad(14)) < 1e-12
  assert np.abs(np.asarray(m.jnt_pos)[m.name2id('ball', 'joint')]).max() > 0
  tb = jacobian.chain_tables(m, TARGETS)
  assert tb['dims'][:5].tolist() == [[6, 7, 14]] * 5 and tb['dims'][:, 2].max() <= jacobian.MAX_CHAIN_DOFS
  assert [jacobian.resolve_target(m, t)['kind'] for t in jc.TARGETS] == ['site', 'body', 'com', 'geom', 'offset']
  sub = jacobian.column_dofs(m, jc.SUBSET)
  assert len(sub) == 11 and list(sub[:4]) == [10, 6, 7, 8]      # out of dof order: the columns follow joint_names
  # the scene stays inside the 10 m the finite-difference bound assumes
  qpos, _ = jc.states(m)
  assert np.abs(qpos).max() < 5


def test_sincos_is_accurate_in_both_precisions():
  x = np.concatenate([np.linspace(-7, 7, 20001), [0.0, np.pi/4, -np.pi/4, np.pi/2, 1e-9, 100.0, -250.0]])
  s, c = emu.sincos(64, x)
  assert max(np.abs(s - np.sin(x)).max(), np.abs(c - np.cos(x)).max()) <= 2.3e-16      # one unit in the last place at 1
  x32 = x.astype(np.float32).astype(np.float64)
  s, c = emu.sincos(32, x32)
  assert max(np.abs(s - np.sin(x32)).max(), np.abs(c - np.cos(x32)).max()) <= 1.2e-7      # one unit in the last place at 1


def test_host_build_equals_the_twin(world):
  """Every target kind, the per-call points, the column subset, the velocity in both frames and the joint forces, over
  all states.  fp64: 1e-9 max(1, |ref|max).  fp32: the worst |J - twin| is MEASURED here and printed; F32_TOL is 4 x it."""
  m = world['m']
  full, sub = jacobian.chain_tables(m, TARGETS), jacobian.chain_tables(m, TARGETS, jc.SUBSET)
  worst = {64: 0.0, 32: 0.0}
  worst_all32 = 0.0
  for s, (q, v, d) in enumerate(zip(world['qpos'], world['qvel'], world['data'])):
    f, tq = _wrench(s)
    pts = _points(s)
    for tables, names in ((full, None), (sub, jc.SUBSET)):
      for point in (None, pts):
        for local in (False, True):
          tw = jc.twin(m, TARGETS, q, v, d['xpos'], d['xquat'], joint_names=names, point=point, local=local, force=f, torque=tq)
          for prec in (64, 32):
            r = emu.run(prec, tables, q, v, point=point, force=f, torque=tq, local=local)
            ej = max(np.abs(r['jacp'] - tw['jacp']).max(), np.abs(r['jacr'] - tw['jacr']).max())
            worst[prec] = max(worst[prec], ej)
            for k in ('jacp', 'jacr', 'vel', 'qfrc'):
              err = np.abs(r[k] - tw[k]).max()
              assert err <= jc.bound(prec, tw[k]), (s, names, point is not None, local, prec, k, err)
              if prec == 32:
                worst_all32 = max(worst_all32, err / max(1.0, np.abs(tw[k]).max()))
  print('worst |J - twin|: fp64 %.3g, fp32 %.3g (F32_MEASURED %.3g, F32_TOL %.3g); fp32 worst scaled error of any output %.3g'
        % (worst[64], worst[32], jc.F32_MEASURED, jc.F32_TOL, worst_all32))
  assert worst[64] <= 1e-13      # the true error sits orders below the bar
  assert worst[32] <= jc.F32_MEASURED and jc.F32_TOL == 4 * jc.F32_MEASURED      # the constant quotes this measurement


def test_off_chain_columns_are_exactly_zero_and_columns_follow_joint_names(world):
  m = world['m']
  full, sub = jacobian.chain_tables(m, TARGETS), jacobian.chain_tables(m, TARGETS, jc.SUBSET)
  q, v = world['qpos'][3], world['qvel'][3]
  for prec in (64, 32):
    r, rs = emu.run(prec, full, q, v), emu.run(prec, sub, q, v)
    for t, ch in enumerate(full['chains']):
      off = np.setdiff1d(np.arange(m.nv), ch['dof_id'])
      assert not r['jacp'][t][:, off].any() and not r['jacr'][t][:, off].any()
      assert np.abs(r['jacp'][t][:, ch['dof_id']]).max() > 0
    np.testing.assert_array_equal(rs['jacp'], r['jacp'][:, :, sub['columns']])      # a subset is a selection: equal bits
    np.testing.assert_array_equal(rs['jacr'], r['jacr'][:, :, sub['columns']])
    np.testing.assert_array_equal(rs['vel'], r['vel'])      # the velocity runs over ALL dofs whatever the columns are


def _quat_conj_mul(a, b):
  return host_data.quat_mul_rows(a * np.array([1.0, -1, -1, -1]), b)


def test_host_build_equals_central_differences_of_the_kinematics(world):
  """Independent of the twin: for every dof k, qpos is moved by +-eps along k (host_data.integrate_pos) and the oracle's
  forward kinematics give the target's displacement and its turn (the local rotation vector of the quaternion
  difference, rotated to the world).  Bound 1e-8: truncation <= eps^2 |r| / 6 ~ 2e-11 |r| and rounding ~ 2^-52 |p| / eps ~
  2e-11 |p| for |r|, |p| <= 10 m."""
  m, eps = world['m'], jc.FD_EPS
  full = jacobian.chain_tables(m, TARGETS)
  tgs = [jacobian.resolve_target(m, t) for t in TARGETS]
  worst = 0.0

  def poses(d):
    xpos, xquat = d['xpos'].reshape(-1, 3), d['xquat'].reshape(-1, 4)
    out = []
    for tg in tgs:
      p, _ = jc.target_frame(m, tg, xpos, xquat)
      out.append((p, host_data.quat_mul_rows(xquat[tg['body']], tg['quat'] / np.linalg.norm(tg['quat']))))
    return out
  on_chain = np.unique(np.concatenate([c['dof_id'] for c in full['chains']]))
  for s in range(jc.NSTATE):      # (16 x 74 x 2 forward passes of the oracle)
    q = world['qpos'][s]
    r = emu.run(64, full, q, world['qvel'][s])
    for k in range(m.nv):
      e = np.zeros(m.nv)
      e[k] = 1.0
      qp, qm = q.copy(), q.copy()
      host_data.integrate_pos(m, qp, e, eps)
      host_data.integrate_pos(m, qm, e, -eps)
      pp, pm = poses(world['forward'](qp)), poses(world['forward'](qm))
      for t in range(T):
        dp = (pp[t][0] - pm[t][0]) / (2 * eps)
        dq = _quat_conj_mul(pm[t][1], pp[t][1])
        if dq[0] < 0:
          dq = -dq
        n = np.linalg.norm(dq[1:])
        rv = dq[1:] * (2 * np.arctan2(n, dq[0]) / n) if n > 0 else np.zeros(3)
        Rm = host_data.quat_to_mat_rows(pm[t][1]).reshape(3, 3)
        dr = Rm @ rv / (2 * eps)
        err = max(np.abs(dp - r['jacp'][t][:, k]).max(), np.abs(dr - r['jacr'][t][:, k]).max())
        worst = max(worst, err)
        assert err <= jc.FD_TOL, (s, k, t, err)
        if k not in on_chain:      # (the column is an exact zero; the difference quotient of a quaternion rounds)
          assert not r['jacp'][t][:, k].any() and not r['jacr'][t][:, k].any() and not dp.any()
  print('worst |J - central difference| %.3g (bound %.1g)' % (worst, jc.FD_TOL))


def test_velocity_equals_object_velocity_from_cvel(world):
  """J qvel against mj_objectVelocity's route through the com-based body velocities (host_data.object_velocity on the
  oracle's cvel / subtree_com): equal analytically."""
  m = world['m']
  full = jacobian.chain_tables(m, TARGETS)
  kinds = dict(site='site', body='xbody', com='body', geom='geom')
  shapes = dict(xpos=(m.nbody, 3), xquat=(m.nbody, 4), xmat=(m.nbody, 3, 3), xipos=(m.nbody, 3), site_xpos=(m.nsite, 3),
                site_xmat=(m.nsite, 3, 3), geom_xpos=(m.ngeom, 3), geom_xmat=(m.ngeom, 3, 3), cvel=(m.nbody, 6), subtree_com=(m.nbody, 3))
  worst = {64: 0.0, 32: 0.0}
  for s, (q, v, d) in enumerate(zip(world['qpos'], world['qvel'], world['data'])):
    get = lambda n, *shape: d[n].reshape(shapes[n])
    for local in (False, True):
      ref = np.zeros((T, 6))
      for t, target in enumerate(TARGETS):
        tg = jacobian.resolve_target(m, target)
        if tg['kind'] == 'offset':      # no object type names it: the body frame's velocity moved along the lever arm
          ang, lin = host_data.object_velocity(m, 'xbody', tg['id'], get, False)
          R = get('xmat')[tg['id']]
          lin = lin + np.cross(ang, R @ tg['pos'])
          if local:
            ang, lin = R.T @ ang, R.T @ lin
        else:
          ang, lin = host_data.object_velocity(m, kinds[tg['kind']], tg['id'], get, local)
        ref[t] = np.concatenate([ang, lin])
      for prec in (64, 32):
        err = np.abs(emu.run(prec, full, q, v, local=local)['vel'] - ref).max()
        worst[prec] = max(worst[prec], err)
        assert err <= jc.bound(prec, ref), (s, local, prec, err)
  print('worst |J qvel - object_velocity|: fp64 %.3g, fp32 %.3g' % (worst[64], worst[32]))


def test_force_is_the_transpose_and_the_seam_agrees(world, monkeypatch):
  import oracle_backend as ob
  from dm_control_amd import mujoco_api as mj
  m = world['m']
  full = jacobian.chain_tables(m, TARGETS)
  s = 5
  q, v, d = world['qpos'][s], world['qvel'][s], world['data'][s]
  f, tq = _wrench(s)
  for prec in (64, 32):
    r = emu.run(prec, full, q, v, force=f, torque=tq)
    ref = np.einsum('tkc,tk->c', r['jacp'], f) + np.einsum('tkc,tk->c', r['jacr'], tq)
    assert np.abs(r['qfrc'] - ref).max() <= jc.bound(prec, ref)
    only = emu.run(prec, full, q, v, force=f)['qfrc']
    assert np.abs(only - np.einsum('tkc,tk->c', r['jacp'], f)).max() <= jc.bound(prec, ref)
    assert not emu.run(prec, full, q, v)['qfrc'].any()
  # the seam: one environment of host numpy on the oracle
  monkeypatch.setattr(mj, 'BatchedPhysics', ob.OracleBatch)
  mm = mj.MjModel.from_xml_string(jc.xml())
  dd = mj.MjData(mm)
  dd.qpos[:] = q
  mj.mj_forward(mm, dd)
  r = emu.run(64, full, q, v, force=f, torque=tq)
  nv = m.nv
  qfrc = np.full(nv, 0.5)
  for t, target in enumerate(TARGETS):
    tg = jacobian.resolve_target(m, target)
    point, _ = jc.target_frame(m, tg, d['xpos'].reshape(-1, 3), d['xquat'].reshape(-1, 4))
    mj.mj_applyFT(mm, dd, f[t], tq[t], point, tg['body'], qfrc)
  assert np.abs(qfrc - 0.5 - r['qfrc']).max() <= 1e-9      # adds in place
  q2 = np.zeros(nv)
  mj.mj_applyFT(mm, dd, f[0], None, np.array(dd.site_xpos[0]) * 1.0, int(m.site_bodyid[0]), q2)
  jp, jr = np.empty((3, nv)), np.empty((3, nv))
  mj.mj_jacSite(mm, dd, jp, jr, 0)
  np.testing.assert_allclose(q2, jp.T @ f[0], atol=1e-14)
  with pytest.raises(mj.FatalError):
    mj.mj_applyFT(mm, dd, f[0], None, np.zeros(3), 1, np.zeros(nv + 1))
  # mj_jacGeom / mj_jacBodyCom / mj_jacPointAxis against mj_jac at the corresponding point
  a, b = np.empty((3, nv)), np.empty((3, nv))
  g = m.name2id('fingertip', 'geom')
  mj.mj_jacGeom(mm, dd, jp, jr, g)
  mj.mj_jac(mm, dd, a, b, np.array(dd.geom_xpos[g]), int(m.geom_bodyid[g]))
  np.testing.assert_array_equal(jp, a)
  np.testing.assert_array_equal(jr, b)
  assert np.abs(jp - r['jacp'][3]).max() <= 1e-9 and np.abs(jr - r['jacr'][3]).max() <= 1e-9
  hand = m.name2id('hand', 'body')
  mj.mj_jacBodyCom(mm, dd, jp, None, hand)
  mj.mj_jac(mm, dd, a, None, np.array(dd.xipos[hand]), hand)
  np.testing.assert_array_equal(jp, a)
  assert np.abs(jp - r['jacp'][2]).max() <= 1e-9
  axis, pt = np.array([0.3, -0.5, 0.8]), np.array([0.2, 0.1, 0.9])
  mj.mj_jacPointAxis(mm, dd, jp, jr, pt, axis, hand)
  mj.mj_jac(mm, dd, a, b, pt, hand)
  np.testing.assert_array_equal(jp, a)
  np.testing.assert_allclose(jr, np.cross(b.T, axis).T, atol=0)
  mj.mj_jacPointAxis(mm, dd, None, jr, pt, axis, hand)      # (either output may be left out)


def test_refusals_are_loud():
  from dm_control_amd import mjcf_compiler as mc
  m = jc.model()
  for bad in ('no_such_site', dict(body='no_such_body'), dict(geom='no_such_geom'), dict(site='x', body='hand'), dict(joint='h1'), 3, None,
              dict(body='hand', com=True, offset=(0, 0, 1)), dict(body='hand', offset=(0, 1)), dict(body=999), dict(geom=-1), dict(body=1.5)):
    with pytest.raises(ValueError):
      jacobian.resolve_target(m, bad)
  with pytest.raises(ValueError, match="'elbow'"):
    jacobian.chain_tables(m, ['grasp'], ['h1', 'elbow'])      # a joint_names entry that is not in the model
  for bad in ('h1', 7, {'h1': 1}):
    with pytest.raises(ValueError, match='joint_names'):
      jacobian.chain_tables(m, ['grasp'], bad)
  with pytest.raises(ValueError, match='twice'):
    jacobian.chain_tables(m, ['grasp'], ['h1', 'h1'])
  with pytest.raises(ValueError, match='at least one target'):
    jacobian.chain_tables(m, [])
  # a target below a mocap body
  mo = mc.compile_xml('<mujoco><worldbody><body name="m" mocap="true" pos="0 0 1"><geom name="mg" size=".1"/><site name="ms"/></body>'
                      '<body name="a"><joint name="j"/><geom size=".1"/><site name="s"/></body></worldbody></mujoco>')
  for t in ('ms', dict(body='m'), dict(geom='mg')):
    with pytest.raises(ValueError, match='mocap'):
      jacobian.chain_tables(mo, [t])
  assert jacobian.chain_tables(mo, ['s'])['dims'].tolist() == [[1, 1, 1]]
  # a chain of more than 64 dofs
  n = 65
  long = mc.compile_xml('<mujoco><worldbody>' + ''.join('<body name="b%d" pos=".01 0 0"><joint name="j%d" axis="0 1 0"/><geom size=".01" mass="1"/>' % (k, k)
                                                         for k in range(n)) + '<site name="tip"/>' + '</body>' * n + '</worldbody></mujoco>')
  with pytest.raises(ValueError, match='65 dofs.*at most 64'):
    jacobian.chain_tables(long, ['tip'])
  assert jacobian.chain_tables(long, [dict(body='b63')])['dims'].tolist() == [[64, 64, 64]]
  # without a batch there is nothing to launch on
  with pytest.raises(TypeError, match='BatchedPhysics'):
    jacobian.BatchJacobian(object(), ['grasp'])
  from dm_control_amd.suite import effector
  with pytest.raises(ValueError, match='targets'):
    effector.wrap(object(), [])
  with pytest.raises(TypeError, match='BatchedPhysics'):
    effector.wrap(object(), ['grasp'])


def test_native_entry_points_validate_without_a_device():
  from dm_control_amd import build
  build.build()
  from dm_control_amd import _native
  with open(os.path.join(ROOT, 'include', 'dmc_jac.h')) as f:
    declared = set(re.findall(r'\b(dmc_jac_[a-z0-9_]+)\s*\(', f.read()))
  assert declared == set(_native.JAC_EXPORTS)
  L = _native.lib()
  assert not [n for n in sorted(declared) if not hasattr(L, n)]
  out = ctypes.c_void_p()
  buf = (ctypes.c_double * 16)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  assert L.dmc_jac_create(None, p, ctypes.byref(out)) != 0 and b'null' in L.dmc_last_error() and not out.value
  assert L.dmc_jac_jacobian(None, None, p, p, None) != 0 and b'null' in L.dmc_last_error()
  assert L.dmc_jac_velocity(None, 0, p, None) != 0 and L.dmc_jac_force(None, p, 0, 0, None, 0, 0, p, None) != 0
  assert L.dmc_jac_info(None, p) != 0
  L.dmc_jac_destroy(None)
  units = {u[0]: u for u in build._UNITS}
  assert 'jac_core.h' in units['jac_kernels.hip'][2] and '-ffp-contract=off' in units['jac_kernels.hip'][1]
  c = emu.caps()
  assert c['max_chain_dofs'] == jacobian.MAX_CHAIN_DOFS == 64 and c['block'] == 64
  for src in ('jac_core.h', 'jac_kernels.hip'):
    with open(os.path.join(build.CSRC, src)) as f:
      text = f.read()
    assert not re.search(r'\basm\b|__asm|atomic[A-Z_(]', text)      # plain arithmetic: no assembly, no atomic call


def test_sanitized_stand_alone_program_over_the_cases(tmp_path, world):
  """csrc/jac_core.h under AddressSanitizer and UBSan: a program with its own main (tests/emu/jac_sanitize.cpp), fed the
  tables and the states as text, in both precisions -- never through Python, never on a GPU."""
  exe = str(tmp_path / 'jac_sanitize')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                         '-Wno-unknown-pragmas', '-o', exe, os.path.join(ROOT, 'tests', 'emu', 'jac_sanitize.cpp')])
  m = world['m']
  tb = jacobian.chain_tables(m, TARGETS, jc.SUBSET)
  C = len(tb['columns'])
  num = lambda a: ' '.join(repr(float(x)) for x in np.asarray(a).ravel())
  lines = ['%d %d %d %d %d %d %d' % (T, C, tb['ints'].size, tb['reals'].size, m.nq, m.nv, jc.NSTATE),
           ' '.join(str(int(x)) for x in tb['dims'].ravel()), ' '.join(str(int(x)) for x in tb['ints']), num(tb['reals'])]
  wrenches = [_wrench(s) for s in range(jc.NSTATE)]
  for s in range(jc.NSTATE):
    lines.append(' '.join([num(world['qpos'][s]), num(world['qvel'][s]), num(wrenches[s][0]), num(wrenches[s][1])]))
  res = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120, check=False)
  assert res.returncode == 0, res.stderr[-2000:]
  rows = [np.array([float(x) for x in l.split()]) for l in res.stdout.strip().split('\n')]
  assert len(rows) == 2 * jc.NSTATE and all(r.shape == (2 + 6*T + C,) for r in rows)
  for s in range(jc.NSTATE):
    for i, prec in enumerate((64, 32)):
      r = emu.run(prec, tb, world['qpos'][s], world['qvel'][s], force=wrenches[s][0], torque=wrenches[s][1], local=s & 1)
      got = rows[2*s + i]
      # (-O1 against the library's -O2, both without contraction: the same IEEE operations)
      np.testing.assert_array_equal(got[2:2 + 6*T], r['vel'].ravel())
      np.testing.assert_array_equal(got[2 + 6*T:], r['qfrc'])
      assert abs(got[0] - np.abs(r['jacp']).sum()) <= 1e-12 * max(1, got[0]) and abs(got[1] - np.abs(r['jacr']).sum()) <= 1e-12 * max(1, got[1])

"""Inverse kinematics without a GPU: the numpy twin (tests/ik_twin.py) against the oracle-backed facade, the host build of
csrc/ik_core.h (tests/emu/ik_emu.cpp) against the twin, and the package's `qpos_from_site_pose` on a single fp64 `Physics`
(the CPU oracle standing in for the device) on the cases of the reference's inverse_kinematics_test.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import ik_cases
import ik_emu_lib
import ik_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [('arm', ik_cases.SITE), ('model_with_ball_joints', ik_cases.SITE), ('chain', 'tip')]


def _xml(name):
  return ik_cases.CHAIN_XML if name == 'chain' else ik_cases.xml(name)


# ---------------------------------------------------------------------------------------------------------------------
# the twin itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,site', MODELS)
def test_twin_kinematics_equal_the_facades(oracle_backend, name, site):
  from dm_control_amd import physics as physics_lib
  p = physics_lib.Physics.from_xml_string(_xml(name))
  tw = ik_twin.Twin(p.model, site)
  sid = p.model.name2id(site, 'site')
  rs = np.random.RandomState(11)
  for _ in range(4):
    q = ik_cases.random_qpos(p.model, rs)
    p.data.qpos = q
    p.forward()
    pos, quat = tw.site_pose(q)
    assert np.abs(pos - np.asarray(p.data.site_xpos)[sid]).max() <= 1e-12
    assert np.abs(ik_twin.qmat(quat).ravel() - np.asarray(p.data.site_xmat)[sid].ravel()).max() <= 1e-12


@pytest.mark.parametrize('name,site', MODELS)
def test_twin_jacobian_equals_central_differences(name, site):
  model = ik_cases.model(name)
  tw = ik_twin.Twin(model, site)
  rs = np.random.RandomState(12)
  eps = 1e-6
  for _ in range(3):
    q = ik_cases.random_qpos(model, rs)
    jp, jr = tw.jacobian(q)
    for d in range(model.nv):
      v = np.zeros(model.nv)
      v[d] = eps
      (p1, q1), (p0, q0) = tw.site_pose(tw.integrate(q, v)), tw.site_pose(tw.integrate(q, -v))
      dp = (p1 - p0) / (2*eps)
      dr = ik_twin.quat_to_vel(ik_twin.qmul(q1, q0*np.array([1.0, -1, -1, -1]))) / (2*eps)
      if not tw.movable[d]:      # (a dof off the chain: integrate leaves it alone, the columns are zero)
        assert not jp[:, d].any() and not jr[:, d].any()
        continue
      assert np.abs(dp - jp[:, d]).max() <= 1e-6, (d, dp, jp[:, d])
      assert np.abs(dr - jr[:, d]).max() <= 1e-6, (d, dr, jr[:, d])


# ---------------------------------------------------------------------------------------------------------------------
# the host build of ik_core.h
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,site', MODELS)
def test_core_kinematics_and_axes_equal_the_twins(name, site):
  model = ik_cases.model(name)
  tw, ch = ik_twin.Twin(model, site), ik_emu_lib.Chain(model, site)
  rs = np.random.RandomState(13)
  for _ in range(4):
    q = ik_cases.random_qpos(model, rs)
    sp, sq, ax, an = ch.pose(q)
    pos, quat, cols = tw._walk(q)      # pylint: disable=protected-access
    assert np.abs(sp - pos).max() <= 1e-14 and np.abs(sq - quat).max() <= 1e-14
    assert sorted(cols) == sorted(int(d) for d in ch.dofs)
    for k, d in enumerate(ch.dofs):
      axis, anchor, rot = cols[int(d)]
      assert np.abs(ax[k] - axis).max() <= 1e-14
      if rot:
        assert np.abs(an[k] - anchor).max() <= 1e-14


def _assert_same(a, b, what):
  assert (a['steps'], a['status']) == (b['steps'], b['status']), (what, a['steps'], a['status'], b['steps'], b['status'])
  assert np.abs(a['qpos'] - b['qpos']).max() <= 1e-9, what


def test_core_fp64_equals_the_twin_on_the_arm():
  model = ik_cases.model('arm')
  tw = ik_twin.Twin(model, ik_cases.SITE, ik_cases.ARM_JOINTS)
  ch = ik_emu_lib.Chain(model, ik_cases.SITE, ik_cases.ARM_JOINTS)
  statuses = set()
  for t, seed, tp, tq, q0 in ik_cases.arm_cases(model):
    a, b = tw.solve(q0, tp, tq, tol=ik_cases.REF_TOL), ch.solve(q0, tp, tq, tol=ik_cases.REF_TOL)
    _assert_same(a, b, (t, seed))
    assert abs(a['err_norm'] - b['err_norm']) <= 1e-12
    statuses.add(a['status'])
  assert statuses == {0, 2}      # converged and progress stops both occur among the 42
  # the step limit
  t, seed, tp, tq, q0 = ik_cases.arm_cases(model)[0]
  a, b = tw.solve(q0, tp, tq, tol=ik_cases.REF_TOL, max_steps=3), ch.solve(q0, tp, tq, tol=ik_cases.REF_TOL, max_steps=3)
  _assert_same(a, b, 'step limit')
  assert (b['steps'], b['status']) == (2, 1)


def test_core_fp64_equals_the_twin_on_ball_and_free_joints():
  rs = np.random.RandomState(14)
  model = ik_cases.model('model_with_ball_joints')
  target = np.array([0.05, 0.05, 0.0])
  for joints, status in ((['joint_1', 'joint_2'], 0), (['joint_1'], 2)):
    tw, ch = ik_twin.Twin(model, ik_cases.SITE, joints), ik_emu_lib.Chain(model, ik_cases.SITE, joints)
    a, b = tw.solve(model.qpos0, target, None, tol=ik_cases.REF_TOL), ch.solve(model.qpos0, target, None, tol=ik_cases.REF_TOL)
    _assert_same(a, b, joints)
    assert b['status'] == status
  model = ik_cases.model('chain')
  for joints in (None, ['h', 'ball'], ['root']):
    tw, ch = ik_twin.Twin(model, 'tip', joints), ik_emu_lib.Chain(model, 'tip', joints)
    for _ in range(4):
      q0 = ik_cases.random_qpos(model, rs)
      goal = tw.site_pose(tw.integrate(q0, np.where(tw.movable, rs.uniform(-0.3, 0.3, model.nv), 0.0)))
      for tp, tq in ((goal[0], None), (goal[0], goal[1])):
        if tq is not None and tw.movable.sum() < 6:
          continue      # (fewer movable dofs than rows: the dual solve's documented singular case)
        a, b = tw.solve(q0, tp, tq, tol=ik_cases.CHAIN_TOL), ch.solve(q0, tp, tq, tol=ik_cases.CHAIN_TOL)
        _assert_same(a, b, (joints, tq is not None))
        fixed = np.ones(model.nq, dtype=bool)
        fixed[ch.qmap[np.repeat(ch.ch['dof_movable'][ch.ch['jnt_dslot']], [(7, 4, 1, 1)[t] for t in ch.ch['jnt_type']]) != 0]] = False
        np.testing.assert_array_equal(b['qpos'][fixed], q0[fixed])


def test_core_fp64_equals_the_twin_on_a_sixty_dof_chain():
  from dm_control_amd import mjcf_compiler
  model = mjcf_compiler.compile_xml(ik_cases.long_chain_xml(20))
  tw, ch = ik_twin.Twin(model, 'end'), ik_emu_lib.Chain(model, 'end')
  assert len(ch.dofs) == 60
  rs = np.random.RandomState(5)
  for _ in range(3):
    q0 = ik_cases.random_qpos(model, rs)
    tp = tw.site_pose(tw.integrate(q0, rs.uniform(-0.05, 0.05, model.nv)))[0]
    a, b = tw.solve(q0, tp, None, tol=ik_cases.CHAIN_TOL), ch.solve(q0, tp, None, tol=ik_cases.CHAIN_TOL)
    _assert_same(a, b, 'long chain')
    assert b['status'] == 0


def test_core_reports_a_singular_pivot():
  """A pose target with one movable hinge: J J' has rank one; without regularisation the factorisation must stop."""
  model = ik_cases.model('arm')
  ch = ik_emu_lib.Chain(model, ik_cases.SITE, ['joint_1'])
  tw = ik_twin.Twin(model, ik_cases.SITE, ['joint_1'])
  q0 = ik_cases.arm_start(model, 0, 0)
  goal = tw.site_pose(tw.integrate(q0, np.where(tw.movable, 0.01, 0.0)))
  r = ch.solve(q0, goal[0], goal[1])
  assert r['status'] == 3 and r['steps'] == 0
  np.testing.assert_array_equal(r['qpos'], q0)


@pytest.mark.parametrize('mode', [1, 2, 3], ids=['pos', 'quat', 'both'])
def test_core_fp32_successes_are_real(mode):
  from dm_control_amd.utils import inverse_kinematics as ik
  model = ik_cases.model('arm')
  tw = ik_twin.Twin(model, ik_cases.SITE, ik_cases.ARM_JOINTS)
  ch = ik_emu_lib.Chain(model, ik_cases.SITE, ik_cases.ARM_JOINTS)
  nok = nwant = 0
  for t, seed, tp, tq, q0 in ik_cases.arm_cases(model):
    if ((1 if tp is not None else 0) | (2 if tq is not None else 0)) != mode:
      continue
    r = ch.solve(q0.astype(np.float32), tp, tq, precision=32, tol=ik.TOL_F32)
    assert r['steps'] <= 100
    nwant += tw.solve(q0, tp, tq, tol=ik.TOL_F32)['status'] == 0
    if r['status'] == 0:
      nok += 1
      assert tw.error(r['qpos'], tp, tq)[1] <= ik.TOL_F32 + ik_cases.KIN_ROUNDING_F32
  assert nwant > 0 and nok >= nwant - 1, (nok, nwant)


def test_fp32_tolerance_is_four_times_the_measured_floor():
  """The derivation of TOL_F32: with tol = 0 the fp32 iteration runs into its floor; the error norms it reports there, over
  the arm's 14 targets from a start the fp64 iteration converges from, stay below the recorded floor."""
  from dm_control_amd.utils import inverse_kinematics as ik
  assert ik.TOL_F32 == 4 * ik.TOL_F32_FLOOR
  model = ik_cases.model('arm')
  tw = ik_twin.Twin(model, ik_cases.SITE, ik_cases.ARM_JOINTS)
  ch = ik_emu_lib.Chain(model, ik_cases.SITE, ik_cases.ARM_JOINTS)
  rs = np.random.RandomState(0)
  floor = 0.0
  for tp, tq in ik_cases.ARM_TARGETS:
    q = np.array(model.qpos0)
    for _ in range(ik_cases.MAX_RESETS + 1):
      if tw.solve(q, tp, tq, tol=ik_cases.REF_TOL)['status'] == 0:
        break
      q = np.array(model.qpos0)
      q[:6] = rs.uniform(0, 2*np.pi, 6)
    floor = max(floor, ch.solve(q, tp, tq, precision=32, tol=0.0)['err_norm'])
  # (another libm's sinf / cosf move the stall point a little: the re-measured floor must stay within a factor of two of the
  # recorded one, i.e. leave at least half of the margin of 4)
  print('fp32 floor re-measured: %.3e (recorded %.3e)' % (floor, ik.TOL_F32_FLOOR))
  assert 0.5*ik.TOL_F32_FLOOR <= floor <= 2*ik.TOL_F32_FLOOR, floor


# ---------------------------------------------------------------------------------------------------------------------
# the package function on a single fp64 Physics
# ---------------------------------------------------------------------------------------------------------------------
class _ResetArm:

  def __init__(self, model):
    self.rs = np.random.RandomState(0)
    self.adr, lo, hi = [], [], []
    for name in ik_cases.ARM_JOINTS:
      j = model.names['joint'].index(name)
      self.adr.append(int(model.jnt_qposadr[j]))
      lo.append(model.jnt_range[j][0] if model.jnt_limited[j] else 0.0)
      hi.append(model.jnt_range[j][1] if model.jnt_limited[j] else 2*np.pi)
    self.lo, self.hi = np.array(lo), np.array(hi)

  def __call__(self, physics):
    q = np.array(physics.data.qpos)
    q[self.adr] = self.rs.uniform(self.lo, self.hi)
    physics.data.qpos = q


@pytest.mark.parametrize('inplace', [False, True])
def test_qpos_from_site_pose_reaches_the_reference_targets(oracle_backend, inplace):
  from dm_control_amd import physics as physics_lib
  from dm_control_amd.utils import inverse_kinematics as ik
  check = physics_lib.Physics.from_xml_string(ik_cases.xml('arm'))
  site = check.model.name2id(ik_cases.SITE, 'site')
  tw = ik_twin.Twin(check.model, ik_cases.SITE)
  for tp, tq in ik_cases.ARM_TARGETS:
    tp, tq = (None if tp is None else np.array(tp)), (None if tq is None else np.array(tq))
    physics = check.copy(share_model=True)
    physics.reset()
    reset, count = _ResetArm(physics.model), 0
    while True:
      before = np.array(physics.data.qpos)
      r = ik.qpos_from_site_pose(physics, ik_cases.SITE, target_pos=tp, target_quat=tq, joint_names=ik_cases.ARM_JOINTS,
                                 tol=ik_cases.REF_TOL, max_steps=100, inplace=inplace)
      if inplace:
        np.testing.assert_array_equal(np.asarray(physics.data.qpos), r.qpos)
      else:
        np.testing.assert_array_equal(np.asarray(physics.data.qpos), before)
      if r.success:
        break
      assert count < ik_cases.MAX_RESETS, 'no solution within %d attempts' % ik_cases.MAX_RESETS
      reset(physics)
      count += 1
    assert r.steps <= 100 and r.err_norm <= ik_cases.REF_TOL
    check.data.qpos = r.qpos
    check.forward()
    if tp is not None:
      np.testing.assert_array_almost_equal(np.asarray(check.data.site_xpos)[site], tp)
    if tq is not None:
      quat = tw.site_pose(r.qpos)[1]
      np.testing.assert_array_almost_equal(ik_twin.qmat(quat), ik_twin.qmat(tq / np.linalg.norm(tq)))
      np.testing.assert_array_almost_equal(np.asarray(check.data.site_xmat)[site].reshape(3, 3), ik_twin.qmat(tq / np.linalg.norm(tq)))


def test_qpos_from_site_pose_indexes_dofs_by_joint(oracle_backend):
  """The ball-joint regression of the reference's test: the target needs both ball joints; the first alone fails."""
  from dm_control_amd import physics as physics_lib
  from dm_control_amd.utils import inverse_kinematics as ik
  physics = physics_lib.Physics.from_xml_string(ik_cases.xml('model_with_ball_joints'))
  target = (0.05, 0.05, 0)
  r = ik.qpos_from_site_pose(physics, ik_cases.SITE, target_pos=target, joint_names=['joint_1', 'joint_2'], tol=ik_cases.REF_TOL,
                             max_steps=100, inplace=True)
  assert r.success and r.steps <= 100 and r.err_norm <= ik_cases.REF_TOL
  np.testing.assert_array_almost_equal(np.asarray(physics.data.site_xpos)[physics.model.name2id(ik_cases.SITE, 'site')], target)
  physics.reset()
  r = ik.qpos_from_site_pose(physics, ik_cases.SITE, target_pos=target, joint_names=['joint_1'], tol=ik_cases.REF_TOL,
                             max_steps=100, inplace=True)
  assert not r.success


@pytest.mark.parametrize('joint_names', [None, ['joint_1', 'joint_2'], ('joint_1', 'joint_2'), np.array(['joint_1', 'joint_2'])],
                         ids=['None', 'list', 'tuple', 'array'])
def test_allowed_joint_name_types(oracle_backend, joint_names):
  from dm_control_amd import physics as physics_lib
  from dm_control_amd.utils import inverse_kinematics as ik
  physics = physics_lib.Physics.from_xml_string(ik_cases.xml('arm'))
  r = ik.qpos_from_site_pose(physics, ik_cases.SITE, target_pos=(0.05, 0.05, 0), joint_names=joint_names, tol=ik_cases.REF_TOL,
                             max_steps=100, inplace=True)
  assert isinstance(r, ik.IKResult) and r.qpos.shape == (physics.model.nq,)


@pytest.mark.parametrize('joint_names', [1, {'joint_1': 1, 'joint_2': 2}, (lambda x: x)], ids=['int', 'dict', 'function'])
def test_refused_joint_name_types(oracle_backend, joint_names):
  from dm_control_amd import physics as physics_lib
  from dm_control_amd.utils import inverse_kinematics as ik
  physics = physics_lib.Physics.from_xml_string(ik_cases.xml('arm'))
  message = ('`joint_names` must be either None, a list, a tuple, or a numpy array; got {}.').format(type(joint_names))
  with pytest.raises(ValueError, match='^' + re.escape(message) + '$'):
    ik.qpos_from_site_pose(physics, ik_cases.SITE, target_pos=(0.05, 0.05, 0), joint_names=joint_names, inplace=True)
  with pytest.raises(ValueError, match='^' + re.escape(message) + '$'):
    ik.extract_chain(physics.model, ik_cases.SITE, joint_names)


def test_a_target_is_required(oracle_backend):
  from dm_control_amd import physics as physics_lib
  from dm_control_amd.utils import inverse_kinematics as ik
  physics = physics_lib.Physics.from_xml_string(ik_cases.xml('arm'))
  with pytest.raises(ValueError, match='^' + re.escape('At least one of `target_pos` or `target_quat` must be specified.') + '$'):
    ik.qpos_from_site_pose(physics, ik_cases.SITE, inplace=True)


def test_nullspace_method():
  from dm_control_amd.utils import inverse_kinematics as ik
  rs = np.random.RandomState(2)
  J, e = rs.normal(size=(6, 9)), rs.normal(size=6)
  np.testing.assert_allclose(ik.nullspace_method(J, e), np.linalg.pinv(J) @ e, atol=1e-9)
  np.testing.assert_allclose(ik.nullspace_method(J, e, 0.03), J.T @ np.linalg.solve(J @ J.T + 0.03*np.eye(6), e), atol=1e-12)


def test_chain_extraction_refuses_what_it_cannot_solve():
  from dm_control_amd.utils import inverse_kinematics as ik
  model = ik_cases.model('chain')
  with pytest.raises(ValueError, match='none of the joints that may move'):
    ik.extract_chain(model, 'tip', ['aside'])
  from dm_control_amd import mjcf_compiler
  long_model = mjcf_compiler.compile_xml(ik_cases.long_chain_xml(22))
  with pytest.raises(ValueError, match='66 dofs'):
    ik.extract_chain(long_model, 'end')


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_ik_header_symbols_are_exported_and_fail_loudly_without_a_batch():
  from dm_control_amd import build
  build.build()
  from dm_control_amd import _native
  with open(os.path.join(ROOT, 'include', 'dmc_ik.h')) as f:
    declared = set(re.findall(r'\b(dmc_ik_[a-z0-9_]+)\s*\(', f.read()))
  assert declared == set(_native.IK_EXPORTS)
  L = _native.lib()
  assert not [n for n in sorted(declared) if not hasattr(L, n)]
  # no CPU fallback: without a batch on a GPU there is no object to solve with, and the entry points say so
  buf = (ctypes.c_double * 64)()
  out = ctypes.c_void_p()
  assert L.dmc_ik_create(None, ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf, ctypes.c_void_p), ctypes.byref(out)) != 0
  assert b'null' in L.dmc_ik_last_error() and not out.value
  p = ctypes.cast(buf, ctypes.c_void_p)
  assert L.dmc_ik_solve(None, p, p, None, 0, p, p, p, p, None) != 0
  assert b'no CPU fallback' in L.dmc_ik_last_error()
  import torch
  if not torch.cuda.is_available():
    from dm_control_amd.batch import BatchedPhysics
    with pytest.raises(_native.NativeError, match='no CPU fallback'):
      BatchedPhysics(ik_cases.model('arm'), 2)


def test_ik_kernels_use_no_scratch():
  """All six instantiations (fp32 / fp64 x position, orientation, both): what an environment indexes at run time is LDS,
  everything else compile-time-indexed registers -- no private segment, no spilled VGPR."""
  import sys
  sys.path.insert(0, os.path.join(ROOT, 'scripts'))
  import kernel_resources
  from dm_control_amd import build
  build.build()
  ks = {n: r for n, r in kernel_resources.kernels(os.path.join(build.CSRC, 'ik_kernels.o')).items() if 'ik_kernel' in n}
  assert len(ks) == 6, sorted(ks)
  for name, r in ks.items():
    assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['vgpr'] <= 256, (name, r)


# ---------------------------------------------------------------------------------------------------------------------
# the `mujoco` seam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,site', MODELS)
def test_seam_jacobians_and_position_integration(monkeypatch, name, site):
  import oracle_backend as ob
  from dm_control_amd import mujoco_api as mj
  monkeypatch.setattr(mj, 'BatchedPhysics', ob.OracleBatch)
  m = mj.MjModel.from_xml_string(_xml(name))
  d = mj.MjData(m)
  model = ik_cases.model(name)
  tw = ik_twin.Twin(model, site)
  sid = model.names['site'].index(site)
  rs = np.random.RandomState(15)
  q = ik_cases.random_qpos(model, rs)
  d.qpos[:] = q
  mj.mj_fwdPosition(m, d)
  jp, jr = np.empty((3, m.nv)), np.empty((3, m.nv))
  mj.mj_jacSite(m, d, jp, jr, sid)
  tp, tr = tw.jacobian(q)
  assert np.abs(jp - tp).max() <= 1e-12 and np.abs(jr - tr).max() <= 1e-12
  jp2, jr2 = np.empty((3, m.nv)), np.empty((3, m.nv))
  mj.mj_jac(m, d, jp2, jr2, np.array(d.site_xpos[sid]), int(model.site_bodyid[sid]))
  np.testing.assert_array_equal(jp2, jp)
  mj.mj_jacSite(m, d, None, jr2, sid)      # (either output may be left out)
  np.testing.assert_array_equal(jr2, jr)
  body = int(model.site_bodyid[sid])
  mj.mj_jacBody(m, d, jp2, jr2, body)
  np.testing.assert_array_equal(jr2, jr)      # same body: same rotation rows; the position rows move with the lever arm
  lever = np.array(d.site_xpos[sid]) - np.array(d.xpos[body])
  assert np.abs(jp2 + np.cross(jr.T, lever).T - jp).max() <= 1e-12
  # mj_integratePos equals the twin's and mj_differentiatePos undoes it
  v = rs.uniform(-0.3, 0.3, m.nv)
  q1 = q.copy()
  mj.mj_integratePos(m, q1, v, 0.5)
  assert np.abs(q1 - tw.integrate(q, np.where(tw.movable, 0.5*v, 0.0)))[tw_entries(model, tw)].max() <= 1e-14
  back = np.zeros(m.nv)
  mj.mj_differentiatePos(m, back, 0.5, q, q1)
  assert np.abs(back - v).max() <= 1e-12


def tw_entries(model, tw):
  """qpos entries of the joints the twin integrates (those on the chain)."""
  keep = np.zeros(model.nq, dtype=bool)
  for j in range(model.njnt):
    if tw.movable[int(model.jnt_dofadr[j])]:
      a = int(model.jnt_qposadr[j])
      keep[a:a + (7, 4, 1, 1)[int(model.jnt_type[j])]] = True
  return keep

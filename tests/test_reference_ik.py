"""The reference's own inverse kinematics -- `dm_control/utils/inverse_kinematics.py` and its test file, imported
unmodified (tests/reference_mujoco.py) -- on this package's `mujoco` seam (mujoco_api.mj_jacSite, mj_integratePos,
mj_fwdPosition) over the fp64 CPU oracle, and the numpy twin (tests/ik_twin.py) held against it."""
import os
import sys

import numpy as np
import pytest

import ik_cases
import ik_twin
import reference_mujoco as rm
import reference_tests

pytestmark = pytest.mark.skipif(not rm.available(), reason='reference tree not present')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def oracle_device(monkeypatch):
  import oracle_backend as ob
  from dm_control_amd import mujoco_api
  monkeypatch.setattr(mujoco_api, 'BatchedPhysics', ob.OracleBatch)


def test_reference_inverse_kinematics_test_passes_on_the_seam(oracle_device):
  """14 targets x inplace, the ball-joint regression, the joint_names type rules and the two error messages."""
  rm.load()
  try:
    result, report = reference_tests.run('utils/inverse_kinematics_test.py', None)
  finally:
    rm.unload()
  assert result.testsRun >= 37, (result.testsRun, report[-3000:])
  assert result.wasSuccessful(), report[-6000:]


@pytest.fixture(scope='module')
def reference_results():
  sys.path.insert(0, os.path.join(ROOT, 'scripts'))
  import make_ik_golden
  return make_ik_golden.reference_results()


def test_twin_takes_the_references_steps(reference_results):
  """Same `steps` and `success` on all 42 cases.  `qpos`: bound = 10 x the largest difference measured here.
  Measured: 6.7e-15 over the 36 cases with a position target.  The 6 orientation-only cases differ by up to 2.4e-3: there
  J'J is a 6 x 6 matrix of rank 3 whose three null singular values (1e-17 .. 3e-16 of the largest) straddle the machine
  precision cut-off of the reference's `lstsq(..., rcond=-1)`, so its step carries a null-space component that the
  dual form's minimum-norm step does not; both reach the target in the same number of steps."""
  model = ik_cases.model('arm')
  tw = ik_twin.Twin(model, ik_cases.SITE, ik_cases.ARM_JOINTS)
  worst = {True: 0.0, False: 0.0}
  for (t, seed, tp, tq, q0), r in reference_results:
    mine = tw.solve(q0, tp, tq, tol=ik_cases.REF_TOL)
    assert (mine['steps'], mine['status'] == 0) == (r.steps, r.success), (t, seed)
    worst[tp is not None] = max(worst[tp is not None], np.abs(mine['qpos'] - r.qpos).max())
  print('max |qpos - reference|: %.3e with a position target, %.3e orientation only' % (worst[True], worst[False]))
  assert worst[True] <= 10 * 6.7e-15
  assert worst[False] <= 10 * 2.4e-3


def test_golden_file_is_what_the_reference_returns(reference_results):
  g = ik_cases.golden()
  assert len(g['cases']) == len(reference_results) == 42
  for c, ((t, seed, tp, tq, q0), r) in zip(g['cases'], reference_results):
    assert (c['target'], c['seed'], c['steps'], c['success']) == (t, seed, r.steps, r.success)
    np.testing.assert_array_equal(np.array(c['qpos0']), q0)
    np.testing.assert_allclose(np.array(c['qpos']), r.qpos, rtol=0, atol=1e-12)
    assert abs(c['err_norm'] - r.err_norm) <= 1e-12

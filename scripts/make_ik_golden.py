"""Records tests/golden/ik_arm_reference.json: what the reference's own `dm_control/utils/inverse_kinematics.py`, imported
unmodified (tests/reference_mujoco.py) and run on the `mujoco` seam of this package over the fp64 CPU oracle, returns for
the arm's 14 test targets from 3 seeded start states each (tests/ik_cases.py).  Needs the reference tree; run from the
repository root:  python scripts/make_ik_golden.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def reference_results():
  """[(case, IKResult)] over ik_cases.arm_cases, from the reference's function."""
  import ik_cases
  import oracle_backend
  import reference_mujoco as rm
  from dm_control_amd import mujoco_api
  saved = mujoco_api.BatchedPhysics
  mujoco_api.BatchedPhysics = oracle_backend.OracleBatch
  try:
    mujoco = rm.load()
    import importlib
    ref_ik = importlib.import_module('dm_control.utils.inverse_kinematics')
    physics = mujoco.Physics.from_xml_string(ik_cases.xml('arm'))
    model = ik_cases.model('arm')
    out = []
    for case in ik_cases.arm_cases(model):
      t, seed, tp, tq, q0 = case
      physics.data.qpos[:] = q0
      r = ref_ik.qpos_from_site_pose(physics, ik_cases.SITE, target_pos=tp, target_quat=tq, joint_names=ik_cases.ARM_JOINTS,
                                     tol=ik_cases.REF_TOL, max_steps=100, inplace=False)
      out.append((case, r))
    return out
  finally:
    rm.unload()
    mujoco_api.BatchedPhysics = saved


def main():
  import ik_cases
  rows = []
  for (t, seed, tp, tq, q0), r in reference_results():
    rows.append(dict(target=t, seed=seed, target_pos=None if tp is None else tp.tolist(),
                     target_quat=None if tq is None else tq.tolist(), qpos0=q0.tolist(), qpos=np.asarray(r.qpos).tolist(),
                     err_norm=float(r.err_norm), steps=int(r.steps), success=bool(r.success)))
  with open(ik_cases.GOLDEN, 'w') as f:
    json.dump(dict(site=ik_cases.SITE, joints=ik_cases.ARM_JOINTS, tol=ik_cases.REF_TOL, max_steps=100, cases=rows), f, indent=1)
  print('wrote %s: %d cases, %d converged' % (ik_cases.GOLDEN, len(rows), sum(r['success'] for r in rows)))


if __name__ == '__main__':
  main()

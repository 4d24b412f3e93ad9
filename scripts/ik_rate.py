"""Solve rate of the batched inverse kinematics (utils/inverse_kinematics.BatchIK) beside the host loop.

  python scripts/ik_rate.py                      every configuration, each in a child process of its own under a time
                                                 limit; writes profiles/ik_rate.json
  python scripts/ik_rate.py --config NAME        one configuration in this process; prints its JSON record

Device configurations: the arm of the reference's test (tests/golden/mujoco_testing_arm.xml, six movable hinges), a
position and an orientation target per environment (the site pose of a seeded random configuration, so every target
is reachable) from seeded random starts; milliseconds per solve launch from HIP events around N back-to-back launches
after a warm-up, solves/s = B / that.  The record keeps how many environments converged and the mean and largest
iteration count: a launch ends with its slowest lane.  Host configuration: `qpos_from_site_pose` on a
single-environment fp64 `Physics`, one call per target (a forward launch and two read-backs per iteration), host clock.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SITE = 'gripsite'
JOINTS = ['joint_%d' % k for k in range(1, 7)]
CONFIGS = {
    'arm_B4096_fp32': dict(B=4096, precision=32), 'arm_B4096_fp64': dict(B=4096, precision=64),
    'arm_B65536_fp32': dict(B=65536, precision=32), 'arm_B65536_fp64': dict(B=65536, precision=64),
    'arm_host_loop_fp64': dict(B=1, precision=64, host=True),
}


def _arm_xml():
  with open(os.path.join(ROOT, 'tests', 'golden', 'mujoco_testing_arm.xml')) as f:
    return f.read()


def _events_ms(torch, fn, reps):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) / reps


def run_config(name, reps):
  import torch
  from dm_control_amd import mjcf_compiler
  from dm_control_amd import physics as physics_lib
  from dm_control_amd.utils import inverse_kinematics as ik
  c = CONFIGS[name]
  B = c['B']
  rec = dict(config=name, B=B, precision=c['precision'])
  if c.get('host'):
    p = physics_lib.Physics.from_xml_string(_arm_xml())
    rs = np.random.RandomState(0)
    n = max(4, reps // 10)
    goals = []
    for _ in range(n):      # reachable targets: the site pose the device reports at a random configuration
      q = np.array(p.model.qpos0)
      q[:6] = rs.uniform(-1, 1, 6)
      p.data.qpos = q
      p.forward()
      goals.append((np.array(p.data.site_xpos[0]), mjcf_compiler.mat_to_quat(np.array(p.data.site_xmat[0]).reshape(3, 3))))
    p.reset()
    ik.qpos_from_site_pose(p, SITE, goals[0][0], goals[0][1], joint_names=JOINTS)
    t0 = time.perf_counter()
    steps, ok = [], 0
    for tp, tq in goals:
      r = ik.qpos_from_site_pose(p, SITE, tp, tq, joint_names=JOINTS)
      steps.append(r.steps)
      ok += bool(r.success)
    dt = time.perf_counter() - t0
    rec.update(solves=n, solves_per_s=n / dt, ms_per_solve=1e3 * dt / n, converged=ok, mean_steps=float(np.mean(steps)),
               max_steps=int(np.max(steps)), tol=ik.TOL_F64)
    return rec
  p = physics_lib.Physics.from_xml_string(_arm_xml(), batch_size=B, precision=c['precision'])
  dev = torch.device('cuda', 0)
  dt = torch.float64 if c['precision'] == 64 else torch.float32
  g = torch.Generator(device='cpu').manual_seed(0)
  nq = p.model.nq
  q0 = torch.tensor(np.tile(p.model.qpos0, (B, 1)))
  goal_q = q0.clone()
  q0[:, :6] = torch.rand((B, 6), generator=g, dtype=torch.float64) * 2 - 1
  goal_q[:, :6] = q0[:, :6] + (torch.rand((B, 6), generator=g, dtype=torch.float64) - 0.5)
  p.batch.set('qpos', goal_q.numpy())
  p.batch.forward(False)
  tp = torch.tensor(np.asarray(p.batch.get('site_xpos')).reshape(B, -1, 3)[:, 0], dtype=dt, device=dev)
  xq = np.asarray(p.batch.get('xquat')).reshape(B, -1, 4)[:, int(p.model.site_bodyid[0])]      # (gripsite has no rotation of its own)
  tq = torch.tensor(xq, dtype=dt, device=dev)
  q0 = q0.to(device=dev, dtype=dt)
  solver = ik.BatchIK(p, SITE, JOINTS)
  for _ in range(5):
    out = solver.solve(tp, tq, qpos=q0)
  torch.cuda.synchronize()
  ms = _events_ms(torch, lambda: solver.solve(tp, tq, qpos=q0), reps)
  steps, status = out['steps'].cpu().numpy(), out['status'].cpu().numpy()
  rec.update(info=solver.info(), tol=solver.tol, ms_per_launch=ms, solves_per_s=B / (ms * 1e-3), converged=int((status == 0).sum()),
             status_counts=[int(x) for x in np.bincount(status, minlength=4)], mean_steps=float(steps.mean()), max_steps=int(steps.max()))
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', default=None)
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--timeout', type=int, default=120)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ik_rate.json'))
  a = ap.parse_args()
  if a.config:
    print('IK_RATE ' + json.dumps(run_config(a.config, a.reps)))
    return 0
  records = []
  for name in CONFIGS:      # one fresh child per configuration, each under its own time limit; stop at the first failure
    cmd = [sys.executable, os.path.abspath(__file__), '--config', name, '--reps', str(a.reps)]
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
      print('%s: time limit of %d s' % (name, a.timeout), file=sys.stderr)
      return 1
    line = [l for l in r.stdout.splitlines() if l.startswith('IK_RATE ')]
    if r.returncode != 0 or not line:
      print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
      return 1
    records.append(json.loads(line[-1][len('IK_RATE '):]))
    print(json.dumps(records[-1]), flush=True)
  doc = dict(device='MI355X', method='HIP events over back-to-back solve launches after warm-up; host loop: host clock',
             records=records)
  with open(a.out, 'w') as f:
    json.dump(doc, f, indent=1)
    f.write('\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

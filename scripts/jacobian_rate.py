"""Rate of the batched Jacobians (jacobian.BatchJacobian) beside the control-step launch of the same batch.

  python scripts/jacobian_rate.py                 every row, each in a child process of its own under a time limit;
                                                  writes profiles/jacobian_rate.json
  python scripts/jacobian_rate.py --config NAME   one row in this process; prints its JSON record

Per row: a batch of B = 4096 environments after a few control steps under random actions; milliseconds per launch from
HIP events around groups of back-to-back launches after a warm-up -- SAMPLES groups of GROUP launches each, the median
over the groups and their spread (min, max).
  walker:      the CMU 2019 walker on the floor (bench.py's config 4), the four end-effector bodies (both hands, both
               feet), C = nv; a control step is 6 physics steps in one launch.
  manipulator: the suite's manipulator, its grasp site, C = nv; a control step is 10 physics steps in one launch.
Measured: one jac() launch (jacp and jacr), one velocity() launch, one force() launch.  Yardstick, in the same process on
the same batch: that control-step launch (Physics.step(n_sub_steps)), whose kernel this unit does not touch.  Also
recorded: the bytes jac() writes and the bytes per second that makes.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {'walker': dict(asset='cmu_2019_position_floor', bench_config=4, nsub=6,
                         targets=[dict(body=b) for b in ('lhand', 'rhand', 'lfoot', 'rfoot')]),
          'manipulator': dict(asset='manipulator', bench_config=None, nsub=10, targets=['grasp'])}
CONFIGS = {'%s_B%d_fp%d' % (s, 4096, p): dict(scene=s, B=4096, precision=p) for s in SCENES for p in (32, 64)}
SAMPLES, GROUP = 40, 10


def _group_ms(torch, fn, samples, group):
  """Milliseconds per launch of `samples` groups of `group` back-to-back launches: (median, min, max)."""
  ms = []
  for _ in range(samples):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(group):
      fn()
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1) / group)
  return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def run_config(name, samples, group):
  import torch
  import bench
  from dm_control_amd import jacobian
  from dm_control_amd.batch import BatchedPhysics, OUT
  from dm_control_amd.suite import common
  c = CONFIGS[name]
  sc = SCENES[c['scene']]
  model = bench.load_model(sc['asset'])
  B, nsub = c['B'], sc['nsub']
  caps = dict(common.DEFAULT_CAPS.get(sc['asset'], {}))
  caps.pop('precision', None)
  b = BatchedPhysics(model, B, precision=c['precision'], **caps)
  if sc['bench_config'] is not None:
    cfg = bench.CONFIGS[sc['bench_config']]
    b.set('qpos', bench.initial_qpos(cfg, model, B, seed0=0, phys=b))
    mask = 0
    for out in cfg['outputs']:
      mask |= OUT[out]
    b.set_output_mask(mask)
  else:      # joint values spread about the model's own start state
    rs = np.random.RandomState(0)
    b.set('qpos', np.asarray(model.qpos0, dtype=np.float64)[None, :] + rs.uniform(-0.2, 0.2, (B, model.nq)))
  b.forward()
  stream = torch.cuda.current_stream().cuda_stream
  dt = torch.float64 if c['precision'] == 64 else torch.float32
  acts = torch.from_numpy(np.random.RandomState(1234).uniform(-1, 1, (model.nu, B))).to(device='cuda', dtype=dt).contiguous()
  b.bind('ctrl', acts.data_ptr())
  step = lambda: b.step(nsub, stream=stream)
  bj = jacobian.BatchJacobian(b, sc['targets'])
  _, T, C = bj.shape
  for _ in range(5):
    step()
  out = list(bj.jac())
  vel = bj.velocity()
  f = torch.ones((B, T, 3), dtype=dt, device='cuda')
  qf = bj.force(f)
  jac = lambda: bj.jac(out=out)
  velocity = lambda: bj.velocity(out=vel)
  force = lambda: bj.force(f, out=qf)
  for _ in range(5):
    jac()
    velocity()
    force()
  torch.cuda.synchronize()
  finite = bool(torch.isfinite(out[0]).all() and torch.isfinite(vel).all() and torch.isfinite(qf).all())
  ms_jac = _group_ms(torch, jac, samples, group)
  ms_vel = _group_ms(torch, velocity, samples, group)
  ms_force = _group_ms(torch, force, samples, group)
  ms_step = _group_ms(torch, step, samples, group)
  torch.cuda.synchronize()
  nbytes = 2 * B * T * 3 * C * (8 if c['precision'] == 64 else 4)
  stat = lambda m: dict(median=m[0], min=m[1], max=m[2])
  return dict(config=name, scene=c['scene'], precision=c['precision'], B=B, targets=T, columns=C, info=bj.info(), finite=finite,
              samples=samples, launches_per_sample=group, ms_per_jac=stat(ms_jac), ms_per_velocity=stat(ms_vel), ms_per_force=stat(ms_force),
              n_sub_steps=nsub, ms_per_control_step=stat(ms_step), jac_output_bytes=nbytes, jac_output_bytes_per_s=nbytes / (ms_jac[0] * 1e-3),
              jac_over_control_step=ms_jac[0] / ms_step[0], velocity_over_control_step=ms_vel[0] / ms_step[0])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', default=None)
  ap.add_argument('--samples', type=int, default=SAMPLES)
  ap.add_argument('--group', type=int, default=GROUP)
  ap.add_argument('--timeout', type=int, default=90)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jacobian_rate.json'))
  a = ap.parse_args()
  if a.samples < 30:
    ap.error('--samples: at least 30 groups')
  if a.config:
    print('JACOBIAN_RATE ' + json.dumps(run_config(a.config, a.samples, a.group)))
    return 0
  records = []
  for name in CONFIGS:      # one fresh child per row, each under its own time limit; stop at the first failure
    cmd = [sys.executable, os.path.abspath(__file__), '--config', name, '--samples', str(a.samples), '--group', str(a.group)]
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
      print('%s: time limit of %d s' % (name, a.timeout), file=sys.stderr)
      return 1
    line = [l for l in r.stdout.splitlines() if l.startswith('JACOBIAN_RATE ')]
    if r.returncode != 0 or not line:
      print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
      return 1
    records.append(json.loads(line[-1][len('JACOBIAN_RATE '):]))
    print(json.dumps(records[-1]), flush=True)
  doc = dict(device='MI355X', method='HIP events around %d groups of %d back-to-back launches after a warm-up, median / min / max over '
             'the groups; one child process per row; the control-step launch of the same batch timed the same way in the same process'
             % (a.samples, a.group), records=records)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(doc, f, indent=1)
    f.write('\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

"""Rate of the batched linearisation (linearize.BatchLinearization.transition) beside the step launches it is made of.

  python scripts/linearize_rate.py                 every row, each in a child process of its own under a time limit;
                                                   writes profiles/linearize_rate.json
  python scripts/linearize_rate.py --config NAME   one row in this process; prints its JSON record

Per row: a batch of B environments after a few control steps under random actions, B chosen so that the scratch batch of
B P environments (P = 1 + 2 (nx + nu) columns per environment) holds about 4096 or about 32768; milliseconds from HIP events
around groups of back-to-back calls after a warm-up -- SAMPLES groups, the median over the groups and their spread (min,
max).  The scenes are bench.py's configs 2, 3 and 4: cheetah (nv = 9, P = 49), humanoid (nv = 27, P = 151) and the CMU 2019
walker on the floor (nv = 62, 56 actuators, P = 361).  fp64 rows: fp64 batch and scratch; fp32 rows: fp32 batch and scratch.
Measured: transition() (A, B; one mj_step per column), against two floors in the same process:
  * step_floor: the bare step(1) launch of the B P environments -- what transition() cannot be faster than; the difference
    is the cost of the fan-out and the differencing.  The cost of a step depends on the states (contacts, solver
    iterations), so the floor steps the very columns transition() steps: the fan-out alone and the fan-out followed by the
    scratch batch's step launch are timed, and the floor is their difference;
  * sequential_floor: P successive step(1) launches of a B-environment batch -- what a user of the parent commit launches
    per linearisation, without the host round trips they would also pay.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('DMC_SPECIALISE', 'cached')      # no kernel build in the background of a timing run

SCENES = {'cheetah': (2, 49), 'humanoid': (3, 151), 'walker': (4, 361)}      # bench.py's config, columns per environment
CONFIGS = {}
for _s, (_c, _p) in SCENES.items():
  for _target in (4096, 32768):
    for _prec in (64, 32):
      _b = max(1, int(round(_target / _p)))
      CONFIGS['%s_B%d_fp%d' % (_s, _b, _prec)] = dict(scene=_s, B=_b, precision=_prec)
SAMPLES, GROUP = 30, 3


def _group_ms(torch, fn, samples, group):
  """Milliseconds per call of `samples` groups of `group` back-to-back calls: (median, min, max)."""
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
  from dm_control_amd import linearize
  from dm_control_amd.batch import BatchedPhysics
  from dm_control_amd.suite import common
  c = CONFIGS[name]
  cfg = bench.CONFIGS[SCENES[c['scene']][0]]
  model = bench.load_model(cfg['asset'])
  B, prec = c['B'], c['precision']
  caps = dict(common.DEFAULT_CAPS.get(cfg['asset'], {}))
  caps.pop('precision', None)
  stream = torch.cuda.current_stream().cuda_stream
  dt = torch.float64 if prec == 64 else torch.float32

  def batch(n):
    b = BatchedPhysics(model, n, precision=prec, **caps)
    b.set('qpos', bench.initial_qpos(cfg, model, n, seed0=0, phys=b))
    b.set_output_mask(0)
    b.legacy_step = False
    acts = torch.from_numpy(np.random.RandomState(1234).uniform(-.5, .5, (model.nu, n))).to(device='cuda', dtype=dt).contiguous()
    b.bind('ctrl', acts.data_ptr())
    for _ in range(5 * cfg['nsub']):
      b.step(1, stream=stream)
    return b, acts

  src, keep0 = batch(B)
  lin = linearize.BatchLinearization(src, precision=prec, eps=1e-6 if prec == 64 else 2.0 ** -10)
  P = lin.P
  assert P == SCENES[c['scene']][1], (P, SCENES[c['scene']])
  seq, keep1 = batch(B)
  out = lin.transition()

  def fan_out_and_step():
    lin.fan_out(stream=stream)
    lin.scratch.step(1, stream=stream)
  calls = dict(transition=lambda: lin.transition(out=out, stream=stream), fan_out=lambda: lin.fan_out(stream=stream),
               fan_out_and_step=fan_out_and_step)

  def sequential():
    for _ in range(P):
      seq.step(1, stream=stream)
  for _ in range(3):
    for fn in calls.values():
      fn()
  sequential()
  torch.cuda.synchronize()
  finite = all(bool(torch.isfinite(t).all()) for t in out)
  warned = int((lin.warnings() != 0).sum().item())
  ms = {k: _group_ms(torch, fn, samples, group) for k, fn in calls.items()}
  ms['sequential_floor'] = _group_ms(torch, sequential, samples, 1)
  torch.cuda.synchronize()
  del keep0, keep1
  stat = lambda m: dict(median=m[0], min=m[1], max=m[2])
  t, f, s = ms['transition'][0], ms['fan_out_and_step'][0] - ms['fan_out'][0], ms['sequential_floor'][0]
  return dict(config=name, scene=c['scene'], precision=prec, B=B, columns=P, scratch_envs=B * P, nv=model.nv, nu=model.nu,
              info=lin.info(), finite=finite, environments_with_warnings=warned, samples=samples, calls_per_sample=group,
              ms={k: stat(v) for k, v in ms.items()}, step_floor_ms=f, transition_over_step_floor=t / f, fan_out_and_difference_ms=t - f,
              fan_out_and_difference_over_step=(t - f) / f, sequential_floor_over_transition=s / t,
              linearisations_per_second=B / (t * 1e-3))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', default=None)
  ap.add_argument('--samples', type=int, default=SAMPLES)
  ap.add_argument('--group', type=int, default=GROUP)
  ap.add_argument('--timeout', type=int, default=120)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linearize_rate.json'))
  a = ap.parse_args()
  if a.samples < 30:
    ap.error('--samples: at least 30 groups')
  if a.config:
    print('LINEARIZE_RATE ' + json.dumps(run_config(a.config, a.samples, a.group)))
    return 0
  records = []
  for name in CONFIGS:      # one fresh child per row, each under its own time limit; stop at the first failure
    cmd = [sys.executable, os.path.abspath(__file__), '--config', name, '--samples', str(a.samples), '--group', str(a.group)]
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
      print('%s: time limit of %d s' % (name, a.timeout), file=sys.stderr)
      return 1
    line = [l for l in r.stdout.splitlines() if l.startswith('LINEARIZE_RATE ')]
    if r.returncode != 0 or not line:
      print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
      return 1
    records.append(json.loads(line[-1][len('LINEARIZE_RATE '):]))
    print(json.dumps(records[-1]), flush=True)
  doc = dict(device='MI355X', method='HIP events around %d groups of %d back-to-back calls after a warm-up (the sequential floor: one '
             'group is its P launches), median / min / max over the groups; one child process per row; both floors timed the same '
             'way in the same process' % (a.samples, a.group), records=records)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(doc, f, indent=1)
    f.write('\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

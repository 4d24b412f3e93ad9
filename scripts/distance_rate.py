"""Rate of the batched geom distances (distance.BatchDistance) beside the control-step launch of the same batch.

  python scripts/distance_rate.py                 every row, each in a child process of its own under a time limit;
                                                  writes profiles/distance_rate.json
  python scripts/distance_rate.py --config NAME   one row in this process; prints its JSON record

Per row: a batch of B environments in the benchmark's start states (bench.py initial_qpos) after a few control steps
under random actions; milliseconds per launch from HIP events around N back-to-back launches after a warm-up.
  soccer: soccer 2v2 BoxHead, the ball against every geom of the four players (28 pairs: boxes, cylinders, capsules, a
          sphere each), B = 256 and 4096; a control step is 5 physics steps in one launch.
  cmu:    the CMU 2019 walker on the floor, both hands (ellipsoids) and both feet (capsules) against the floor and --
          the asset holds no target prop -- against each other (4 plane pairs + 6 convex pairs), B = 4096; a control step
          is 6 physics steps in one launch.
Yardstick, in the same process on the same batch: that control-step launch (Physics.step(n_sub_steps)), whose kernel this
unit does not touch.  Also recorded: the share of lanes in which a geom pair's cores overlapped (EPA ran) and the share
that reported a cap.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAYERS = ('home0', 'home1', 'away0', 'away1')
SCENES = {'soccer': dict(bench_config=5), 'cmu': dict(bench_config=4)}
CONFIGS = {'%s_B%d_fp%d' % (s, B, p): dict(scene=s, B=B, precision=p)
           for s, B in (('soccer', 256), ('soccer', 4096), ('cmu', 4096)) for p in (32, 64)}


def scene_pairs(scene, model):
  names = model.names['geom']
  if scene == 'soccer':
    return [('soccer_ball/geom', n) for n in names if n is not None and n.split('/')[0] in PLAYERS]
  limbs = ['lhand', 'rhand', 'lfoot', 'rfoot']
  return [(n, 'groundplane') for n in limbs] + [(a, b) for i, a in enumerate(limbs) for b in limbs[i + 1:]]


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
  import bench
  from dm_control_amd import distance
  from dm_control_amd.batch import BatchedPhysics, OUT
  from dm_control_amd.suite import common
  c = CONFIGS[name]
  cfg = bench.CONFIGS[SCENES[c['scene']]['bench_config']]
  model = bench.load_model(cfg['asset'])
  B, nsub = c['B'], cfg['nsub']
  caps = dict(common.DEFAULT_CAPS.get(cfg['asset'], {}))
  caps.pop('precision', None)
  b = BatchedPhysics(model, B, precision=c['precision'], **caps)
  b.set('qpos', bench.initial_qpos(cfg, model, B, seed0=0, phys=b))
  mask = OUT['geom']
  for out in cfg['outputs']:
    mask |= OUT[out]
  b.set_output_mask(mask)
  b.forward()
  stream = torch.cuda.current_stream().cuda_stream
  dt = torch.float64 if c['precision'] == 64 else torch.float32
  acts = torch.from_numpy(np.random.RandomState(1234).uniform(-1, 1, (model.nu, B))).to(device='cuda', dtype=dt).contiguous()
  b.bind('ctrl', acts.data_ptr())
  step = lambda: b.step(nsub, stream=stream)
  pairs = scene_pairs(c['scene'], model)
  bd = distance.BatchDistance(b, pairs, distmax=10.0)
  for _ in range(5):
    step()
  out = list(bd.query(fromto=True, normal=True, status='bits'))
  full = lambda: bd.query(fromto=True, normal=True, status='bits', out=out)
  dist_only = lambda: bd.query(out=out[:1])
  for _ in range(5):
    full()
    dist_only()
  torch.cuda.synchronize()
  bits = out[3].clone()
  ms_full = _events_ms(torch, full, reps)
  ms_dist = _events_ms(torch, dist_only, reps)
  ms_step = _events_ms(torch, step, reps)
  torch.cuda.synchronize()
  return dict(config=name, scene=c['scene'], precision=c['precision'], B=B, pairs=len(pairs), lanes=B*len(pairs), info=bd.info(),
              epa_lane_share=float(((bits >> 1) & 1).float().mean()), cap_lane_share=float((bits & 1).float().mean()),
              min_dist=float(out[0].min()), ms_per_query=ms_full, ms_per_query_dist_only=ms_dist, pairs_per_s=B*len(pairs)/(ms_full*1e-3),
              n_sub_steps=nsub, ms_per_control_step=ms_step, query_over_control_step=ms_full/ms_step)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', default=None)
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--timeout', type=int, default=90)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'distance_rate.json'))
  a = ap.parse_args()
  if a.config:
    print('DISTANCE_RATE ' + json.dumps(run_config(a.config, a.reps)))
    return 0
  records = []
  for name in CONFIGS:      # one fresh child per row, each under its own time limit; stop at the first failure
    cmd = [sys.executable, os.path.abspath(__file__), '--config', name, '--reps', str(a.reps)]
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
      print('%s: time limit of %d s' % (name, a.timeout), file=sys.stderr)
      return 1
    line = [l for l in r.stdout.splitlines() if l.startswith('DISTANCE_RATE ')]
    if r.returncode != 0 or not line:
      print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
      return 1
    records.append(json.loads(line[-1][len('DISTANCE_RATE '):]))
    print(json.dumps(records[-1]), flush=True)
  doc = dict(device='MI355X', method='HIP events over %d back-to-back launches after a warm-up; one child process per row; the '
             'control-step launch of the same batch timed the same way in the same process' % a.reps, records=records)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(doc, f, indent=1)
    f.write('\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

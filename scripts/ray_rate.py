"""Rate of the batched ray casts (rays.BatchRays) beside the camera kernel rendering depth only on the same batch.

  python scripts/ray_rate.py                      every row, each in a child process of its own under a time limit;
                                                  writes profiles/ray_rate.json
  python scripts/ray_rate.py --config NAME        one row in this process; prints its JSON record

Per row: a batch of B environments of the model after one forward launch; milliseconds per launch from HIP events around
N back-to-back launches after a warm-up; rays/s = B R / that.  cast: R seeded directions per environment from the
origin of a body of the model, read back once.  scan: a ring table of R directions in that body's frame.  Yardstick, in the
same process on the same batch: the existing camera kernel rendering depth only from a fixed camera on the same body with
H W = R pixels (the camera culls per tile and sees its own body; the rays skip it).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {'cheetah': dict(asset='cheetah.xml', body='torso', kw={}),
          'soccer': dict(asset='soccer_2v2_boxhead.xml', body='home0/torso', kw=dict(nconmax=24))}
SHAPES = {1: (1, 1), 64: (8, 8), 256: (16, 16), 1024: (32, 32)}
CONFIGS = {'%s_fp%d_%s_R%d' % (m, p, kind, R): dict(model=m, precision=p, kind=kind, R=R, B=4096)
           for m in MODELS for p in (32, 64) for kind, R in (('cast', 1), ('cast', 64), ('scan', 256), ('scan', 1024))}


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
  from dm_control_amd import camera, mjcf_compiler, rays
  from dm_control_amd.batch import BatchedPhysics
  c = CONFIGS[name]
  spec = MODELS[c['model']]
  with open(os.path.join(ROOT, 'dm_control_amd', 'suite', 'assets', spec['asset'])) as f:
    model = mjcf_compiler.compile_xml(f.read())
  B, R = c['B'], c['R']
  b = BatchedPhysics(model, B, precision=c['precision'], **spec['kw'])
  b.forward()
  b.sync()
  dt = torch.float64 if c['precision'] == 64 else torch.float32
  body = model.name2id(spec['body'], 'body')
  br = rays.BatchRays(b)
  if c['kind'] == 'cast':
    rs = np.random.RandomState(0)
    vec = rs.normal(size=(B, R, 3))
    vec /= np.linalg.norm(vec, axis=2, keepdims=True)
    pnt = torch.tensor(np.repeat(b.get('xpos').reshape(B, -1, 3)[:, body][:, None], R, 1), dtype=dt, device='cuda')
    vec = torch.tensor(vec, dtype=dt, device='cuda')
    out = br.cast(pnt, vec, bodyexclude=body)
    fn = lambda: br.cast(pnt, vec, bodyexclude=body, out=out)
  else:
    n_el = 4 if R >= 256 else 1
    br.add_scan(dict(body=spec['body']), rays.ring(R // n_el, elevations=np.linspace(-0.6, 0.3, n_el)))
    out = br.scan()
    fn = lambda: br.scan(out=out)
  H, W = SHAPES[R]
  cam = camera.BatchCamera(b, [dict(body=spec['body'], xyaxes=(0, -1, 0, 0, 0, 1), fovy=90)], H, W)
  depth = cam.render(depth=True)
  for _ in range(5):
    fn()
    cam.render(depth=True, out=depth)
  torch.cuda.synchronize()
  ms = _events_ms(torch, fn, reps)
  cam_ms = _events_ms(torch, lambda: cam.render(depth=True, out=depth), reps)
  hits = float((out[1] >= 0).float().mean())
  return dict(config=name, model=c['model'], precision=c['precision'], kind=c['kind'], B=B, R=R, info=br.info(), hit_share=hits,
              ms_per_launch=ms, rays_per_s=B * R / (ms * 1e-3), camera_hw=[H, W], camera_depth_ms_per_launch=cam_ms,
              camera_rays_per_s=B * R / (cam_ms * 1e-3), camera_ms_over_rays_ms=cam_ms / ms)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', default=None)
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--timeout', type=int, default=90)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ray_rate.json'))
  a = ap.parse_args()
  if a.config:
    print('RAY_RATE ' + json.dumps(run_config(a.config, a.reps)))
    return 0
  records = []
  for name in CONFIGS:      # one fresh child per row, each under its own time limit; stop at the first failure
    cmd = [sys.executable, os.path.abspath(__file__), '--config', name, '--reps', str(a.reps)]
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
      print('%s: time limit of %d s' % (name, a.timeout), file=sys.stderr)
      return 1
    line = [l for l in r.stdout.splitlines() if l.startswith('RAY_RATE ')]
    if r.returncode != 0 or not line:
      print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
      return 1
    records.append(json.loads(line[-1][len('RAY_RATE '):]))
    print(json.dumps(records[-1]), flush=True)
  doc = dict(device='MI355X', method='HIP events over %d back-to-back launches after a warm-up; one child process per row' % a.reps,
             records=records)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(doc, f, indent=1)
    f.write('\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

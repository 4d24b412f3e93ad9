"""Render rate of the ray-cast cameras (camera.BatchCamera) beside the step launch of the same batch.

  python scripts/camera_rate.py                      every configuration, each in a child process of its own under a
                                                     time limit; writes profiles/camera_rate.json
  python scripts/camera_rate.py --config NAME        one configuration in this process; prints its JSON record

Per configuration: milliseconds per render launch (HIP events around N back-to-back launches after a warm-up), with the
per-tile geom cull on and off and with the LDS pre-transform off; milliseconds per control-step launch of the same batch (dmc_batch_time_steps, HIP events);
env-steps/s of the environment's step loop without pixels and wrapped by suite/pixels.py (host clock around a loop that
ends in a device synchronise).  The render is also timed without the per-(camera, geom) pre-transform (the world frame
staged, transformed per pixel).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EGO = ['home0/egocentric', 'home1/egocentric', 'away0/egocentric', 'away1/egocentric']
CONFIGS = {
    'cheetah_B4096_84x84_trackcom': dict(kind='fused', domain='cheetah', task='run', B=4096, hw=(84, 84),
                                         cameras=[dict(body='torso', pos=(0, -3, 0.5), xyaxes=(1, 0, 0, 0, 0, 1), mode='trackcom')]),
    'soccer_2v2_B256_4x64x64_egocentric': dict(kind='composer', name='soccer_2v2', B=256, hw=(64, 64), cameras=EGO),
    'soccer_2v2_B4096_4x64x64_egocentric': dict(kind='composer', name='soccer_2v2', B=4096, hw=(64, 64), cameras=EGO),
    'cmu_walker_B4096_64x64_egocentric': dict(kind='composer', name='cmu_go_to_target', B=4096, hw=(64, 64),
                                              cameras=[dict(body='head', pos=(0, 0.1, 0.1), xyaxes=(-1, 0, 0, 0, 1, 0), fovy=80)]),
}


def _events_ms(torch, fn, reps):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) / reps


def _loop_rate(torch, env, act, steps, B):
  for _ in range(10):
    env.step(act)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(steps):
    env.step(act)
  torch.cuda.synchronize()
  return B * steps / (time.perf_counter() - t0)


def run_config(name, reps, steps):
  import torch
  from dm_control_amd.suite import pixels
  c = CONFIGS[name]
  B, (H, W) = c['B'], c['hw']
  if c['kind'] == 'fused':
    from dm_control_amd.suite import fused_env
    env = fused_env.make(c['domain'], c['task'], B)
    n_sub = env.n_sub_steps
    nu = env.model.nu
    dtype = env.dtype
  else:
    from dm_control_amd import composer
    env = composer.make(c['name'], B)
    n_sub = env.n_sub_steps
    nu = env.physics.batch.model.nu
    dtype = torch.float32
  cams = c['cameras']
  env.reset()
  act = torch.zeros((B, nu), dtype=dtype, device='cuda').uniform_(-1, 1)
  rec = dict(config=name, B=B, height=H, width=W, ncam=len(cams), n_sub_steps=int(n_sub))
  rec['env_steps_per_s_no_pixels'] = _loop_rate(torch, env, act, steps, B)
  penv = pixels.wrap(env, cams, H, W)
  cam, batch = penv.camera, penv.camera.batch
  rec['ngeom'] = int(batch.model.ngeom)
  rec['skipped_geoms'] = len(cam.skipped_geoms)
  penv.reset()
  for _ in range(20):
    penv.step(act)
  out = cam.render()
  # A/B of the two kernel choices, interleaved twice so that a drift of the clock shows as a spread between the rounds
  variants = (('cull_on', dict()), ('cull_off', dict(cull=False)), ('pretransform_off', dict(pretransform=False)))
  for rnd in range(2):
    for label, kw in variants:
      cam.set_tuning(**kw)
      for _ in range(10):
        cam.render(out=out)
      rec.setdefault('render_ms_rgb_' + label, []).append(_events_ms(torch, lambda: cam.render(out=out), reps))
  cam.set_tuning()
  for label, _ in variants:
    rec['render_ms_rgb_%s_rounds' % label] = rec['render_ms_rgb_' + label]
    rec['render_ms_rgb_' + label] = min(rec['render_ms_rgb_' + label])
  depth = cam.render(depth=True)
  rec['render_ms_depth'] = _events_ms(torch, lambda: cam.render(depth=True, out=depth), reps)
  rec['render_ms_all_three'] = _events_ms(torch, cam.render_all, reps)
  rec['images_per_s_rgb'] = B * len(cams) / (rec['render_ms_rgb_cull_on'] * 1e-3)
  torch.cuda.synchronize()
  batch.time_steps(n_sub, 5)
  rec['step_launch_ms'] = float(batch.time_steps(n_sub, max(10, reps // 4)))
  rec['env_steps_per_s_pixels'] = _loop_rate(torch, penv, act, steps, B)
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', default=None)
  ap.add_argument('--reps', type=int, default=200)
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--timeout', type=int, default=240)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'camera_rate.json'))
  a = ap.parse_args()
  if a.config:
    print('CAMERA_RATE ' + json.dumps(run_config(a.config, a.reps, a.steps)))
    return 0
  records = []
  for name in CONFIGS:      # one fresh child per configuration, each under its own time limit; stop at the first failure
    cmd = [sys.executable, os.path.abspath(__file__), '--config', name, '--reps', str(a.reps), '--steps', str(a.steps)]
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
      print('%s: time limit of %d s' % (name, a.timeout), file=sys.stderr)
      return 1
    line = [l for l in r.stdout.splitlines() if l.startswith('CAMERA_RATE ')]
    if r.returncode != 0 or not line:
      print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
      return 1
    records.append(json.loads(line[-1][len('CAMERA_RATE '):]))
    print(json.dumps(records[-1]), flush=True)
  doc = dict(device='MI355X', method='HIP events over back-to-back launches after warm-up; loops: host clock to a device synchronise',
             records=records)
  if os.path.exists(a.out):      # (scripts/camera_texture_rate.py keeps its measurement in the same file)
    with open(a.out) as f:
      doc.update({k: v for k, v in json.load(f).items() if k == 'textures'})
  with open(a.out, 'w') as f:
    json.dump(doc, f, indent=1)
    f.write('\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

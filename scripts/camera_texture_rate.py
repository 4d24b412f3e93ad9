"""What the camera's textures cost: cheetah, B = 4096, one 84 x 84 trackcom RGB camera (the README's pixel example).

  python scripts/camera_texture_rate.py [--parent-variant NAME]     every state twice, interleaved, each in a child process
                                                                   of its own under a time limit; merges the result into
                                                                   profiles/camera_rate.json under "textures"
  python scripts/camera_texture_rate.py --state STATE               one state in this process; prints its JSON record

States: `off` (no texture argument: the flat-colour kernel), `nearest` and `box` (the suite's grid floor and skybox,
camera.SUITE_GRID / SUITE_SKYBOX), and `parent`: `off` run on libdmc_hip_NAME.so, a build of the commit before the textures
(python dm_control_amd/build.py --variant=NAME in a checkout of that commit, the library copied next to this one's) -- the
textures-off kernel is meant to be that kernel, so the two must agree within the spread of the two rounds.
Per state: milliseconds per RGB render launch (HIP events around back-to-back launches after a warm-up, the smaller of two
in-process rounds) and env-steps/s of the pixels.wrap step loop (host clock to a device synchronise).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

B, HW = 4096, (84, 84)
CAMERA = dict(body='torso', pos=(0, -3, 0.5), xyaxes=(1, 0, 0, 0, 0, 1), mode='trackcom')
STATES = ('parent', 'off', 'nearest', 'box')


def run_state(state, reps, steps):
  import torch
  import camera_rate
  from dm_control_amd import camera
  from dm_control_amd.suite import fused_env, pixels
  kw = {} if state in ('parent', 'off') else dict(materials={'ground': camera.SUITE_GRID}, skybox=camera.SUITE_SKYBOX, texture_filter=state)
  env = fused_env.make('cheetah', 'run', B)
  penv = pixels.wrap(env, [CAMERA], *HW, **kw)
  cam = penv.camera
  penv.reset()
  act = torch.zeros((B, env.model.nu), dtype=env.dtype, device='cuda').uniform_(-1, 1)
  for _ in range(20):
    penv.step(act)
  out = cam.render()
  ms = []
  for _ in range(2):
    for _ in range(10):
      cam.render(out=out)
    ms.append(camera_rate._events_ms(torch, lambda: cam.render(out=out), reps))
  return dict(state=state, B=B, height=HW[0], width=HW[1], render_ms_rgb=min(ms), render_ms_rgb_rounds=ms,
              env_steps_per_s_pixels=camera_rate._loop_rate(torch, penv, act, steps, B))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--state', default=None, choices=STATES)
  ap.add_argument('--parent-variant', default=None)
  ap.add_argument('--reps', type=int, default=200)
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--timeout', type=int, default=120)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'camera_rate.json'))
  a = ap.parse_args()
  if a.state:
    print('CAMERA_TEXTURE_RATE ' + json.dumps(run_state(a.state, a.reps, a.steps)))
    return 0
  states = [s for s in STATES if s != 'parent' or a.parent_variant]
  rounds = []
  for rnd in range(2):      # interleaved: a drift of the clock shows as a spread between the rounds
    rounds.append({})
    for state in states:      # one fresh child per state, each under its own time limit; stop at the first failure
      env = dict(os.environ)
      if state == 'parent':
        env['DMC_LIB_VARIANT'] = a.parent_variant
      cmd = [sys.executable, os.path.abspath(__file__), '--state', state, '--reps', str(a.reps), '--steps', str(a.steps)]
      try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
      except subprocess.TimeoutExpired:
        print('%s: time limit of %d s' % (state, a.timeout), file=sys.stderr)
        return 1
      line = [l for l in r.stdout.splitlines() if l.startswith('CAMERA_TEXTURE_RATE ')]
      if r.returncode != 0 or not line:
        print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
        return 1
      rounds[-1][state] = json.loads(line[-1][len('CAMERA_TEXTURE_RATE '):])
      print(json.dumps(rounds[-1][state]), flush=True)
  summary = {}
  for state in states:
    ms = [r[state]['render_ms_rgb'] for r in rounds]
    summary[state] = dict(render_ms_rgb=min(ms), render_ms_rgb_rounds=ms,
                          env_steps_per_s_pixels=max(r[state]['env_steps_per_s_pixels'] for r in rounds),
                          env_steps_per_s_pixels_rounds=[r[state]['env_steps_per_s_pixels'] for r in rounds])
  if 'parent' in summary:
    p, o = summary['parent']['render_ms_rgb_rounds'], summary['off']['render_ms_rgb_rounds']
    summary['off_vs_parent'] = dict(relative_difference=summary['off']['render_ms_rgb'] / summary['parent']['render_ms_rgb'] - 1,
                                    rounds_disagree_by=max(abs(p[0] / p[1] - 1), abs(o[0] / o[1] - 1)))
  doc = {}
  if os.path.exists(a.out):
    with open(a.out) as f:
      doc = json.load(f)
  doc['textures'] = dict(config='cheetah_B4096_84x84_trackcom', method='two interleaved rounds of one child process per state; HIP events over '
                         'back-to-back launches after warm-up; loop: host clock to a device synchronise', states=summary)
  with open(a.out, 'w') as f:
    json.dump(doc, f, indent=1)
    f.write('\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

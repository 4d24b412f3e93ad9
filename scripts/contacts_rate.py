"""Rate of the batched contact wrenches (contacts.BatchContacts) beside the control-step launch of the same batch.

  python scripts/contacts_rate.py                 every row, each in a child process of its own under a time limit;
                                                  writes profiles/contacts_rate.json
  python scripts/contacts_rate.py --config NAME   one row in this process; prints its JSON record

Per row: a batch of B = 4096 environments after a few control steps under random actions; milliseconds per launch from
HIP events around groups of back-to-back launches after a warm-up -- SAMPLES groups of GROUP launches each, the median
over the groups and their spread (min, max).  The scenes are bench.py's configs 4 and 5: the CMU 2019 walker on the floor
(its two feet against the ground plane, T = 2) and soccer 2v2 (the ball against each of the four players' subtrees,
T = 4), in fp32.
Measured: one launch each of net_all() and wrench(), and refresh() -- a forward launch between two device-to-device
copies of the warm start.  Yardstick, in the same process on the same batch: the control-step launch
(Physics.step(n_sub_steps)) with the output mask the unit needs, whose kernel this unit does not touch.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {'walker': 4, 'soccer': 5}      # bench.py's configs
CONFIGS = {'%s_B%d_fp%d' % (s, 4096, 32): dict(scene=s, B=4096, precision=32) for s in SCENES}
CALLS = ('net_all', 'wrench', 'refresh')
SAMPLES, GROUP = 40, 10


def targets(scene, model):
  names = [n for n in model.names['geom'] if n]
  if scene == 'walker':
    ground = [n for n in names if 'ground' in n][0]
    return [dict(geom=[n for n in names if side + 'foot' in n and 'touch' not in n], other=ground) for side in 'lr']
  players = [n for n in model.names['body'] if n and n.endswith('/') and n[:4] in ('home', 'away') and 'goal' not in n]
  return [dict(body='soccer_ball/', other=dict(body=p, subtree=True)) for p in players]


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
  from dm_control_amd import contacts
  from dm_control_amd.batch import BatchedPhysics, OUT
  from dm_control_amd.suite import common
  c = CONFIGS[name]
  cfg = bench.CONFIGS[SCENES[c['scene']]]
  model = bench.load_model(cfg['asset'])
  B, nsub = c['B'], cfg['nsub']
  caps = dict(common.DEFAULT_CAPS.get(cfg['asset'], {}))
  caps.pop('precision', None)
  b = BatchedPhysics(model, B, precision=c['precision'], **caps)
  b.set('qpos', bench.initial_qpos(cfg, model, B, seed0=0, phys=b))
  tg = targets(c['scene'], model)
  bc = contacts.BatchContacts(b, tg)
  mask = bc.output_mask
  for out in cfg['outputs']:
    mask |= OUT[out]
  b.set_output_mask(mask)
  b.forward()
  stream = torch.cuda.current_stream().cuda_stream
  dt = torch.float64 if c['precision'] == 64 else torch.float32
  acts = torch.from_numpy(np.random.RandomState(1234).uniform(-1, 1, (model.nu, B))).to(device='cuda', dtype=dt).contiguous()
  b.bind('ctrl', acts.data_ptr())
  step = lambda: b.step(nsub, stream=stream)
  for _ in range(5):
    step()
  bc.refresh()
  out, w = bc.net_all(), bc.wrench()
  calls = dict(net_all=lambda: bc.net_all(out=out), wrench=lambda: bc.wrench(out=w), refresh=bc.refresh)
  for _ in range(5):
    for fn in calls.values():
      fn()
  torch.cuda.synchronize()
  finite = bool(torch.isfinite(out['force']).all()) and bool(torch.isfinite(w).all())
  touching = float((out['count'] > 0).float().mean())
  ms = {k: _group_ms(torch, calls[k], samples, group) for k in CALLS}
  ms_step = _group_ms(torch, step, samples, group)
  torch.cuda.synchronize()
  stat = lambda m: dict(median=m[0], min=m[1], max=m[2])
  return dict(config=name, scene=c['scene'], precision=c['precision'], B=B, ntarget=len(tg), info=bc.info(), finite=finite,
              targets_in_contact=touching, mean_ncon=float(np.mean(b.get('ncon'))), samples=samples, launches_per_sample=group,
              n_sub_steps=nsub, ms_per_control_step=stat(ms_step), ms_per_call={k: stat(ms[k]) for k in CALLS},
              over_control_step={k: ms[k][0] / ms_step[0] for k in CALLS})


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', default=None)
  ap.add_argument('--samples', type=int, default=SAMPLES)
  ap.add_argument('--group', type=int, default=GROUP)
  ap.add_argument('--timeout', type=int, default=90)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'contacts_rate.json'))
  a = ap.parse_args()
  if a.samples < 30:
    ap.error('--samples: at least 30 groups')
  if a.config:
    print('CONTACTS_RATE ' + json.dumps(run_config(a.config, a.samples, a.group)))
    return 0
  records = []
  for name in CONFIGS:      # one fresh child per row, each under its own time limit; stop at the first failure
    cmd = [sys.executable, os.path.abspath(__file__), '--config', name, '--samples', str(a.samples), '--group', str(a.group)]
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
      print('%s: time limit of %d s' % (name, a.timeout), file=sys.stderr)
      return 1
    line = [l for l in r.stdout.splitlines() if l.startswith('CONTACTS_RATE ')]
    if r.returncode != 0 or not line:
      print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
      return 1
    records.append(json.loads(line[-1][len('CONTACTS_RATE '):]))
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

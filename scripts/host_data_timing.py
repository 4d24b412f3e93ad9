"""Host time of the derived mjData arrays, this tree against another revision, on the fp64 oracle stand-in (no GPU: the
code is host numpy, and the stand-in takes the launch out of the number).

  python scripts/host_data_timing.py --parent HEAD [--out profiles/host_data_timing.json]

extracts `--parent` with `git archive`, then runs parent and tree interleaved, RUNS child processes each
(`--measure --root DIR`); every child reports the median of REPS repetitions per leg:

  a            `mj_step` of an `MjData` on humanoid with xanchor, M and ten_length handed out.  That path's code only
               moved: the tree's medians must lie within the parent's own min-max spread, widened by that spread once.
  b            `physics.data.xanchor` after `forward()` at B = 64 on humanoid (only the read is timed): not slower than
               the parent -- it replaces an O(B * nbody) Python loop.
  c_<model>    the same read at B = 1 on cartpole and humanoid_CMU: no bound, recorded.  The per-rank pass has a fixed numpy
               cost that a two-joint model does not amortise; nothing in the package reads xanchor / xaxis per step.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS, REPS = 3, 200


def measure(root):
  sys.path[:0] = [root, os.path.join(root, 'tests')]
  import oracle_backend
  from dm_control_amd import mujoco_api as mj
  from dm_control_amd import physics
  from dm_control_amd.suite import common
  mj.BatchedPhysics = physics.BatchedPhysics = oracle_backend.OracleBatch

  def median(setup, timed):
    times = []
    for _ in range(REPS + 10):
      setup()
      t0 = time.perf_counter()
      timed()
      times.append(time.perf_counter() - t0)
    return statistics.median(times[10:])
  out = {}
  m = mj.MjModel.from_xml_string(common.read_model('humanoid.xml'))
  d = mj.MjData(m)
  mj.mj_forward(m, d)
  d.xanchor, d.M, d.ten_length      # pylint: disable=pointless-statement  (handed out: refreshed after every launch)
  out['a'] = median(lambda: None, lambda: mj.mj_step(m, d))
  for leg, model, batch in (('b', 'humanoid', 64), ('c_cartpole', 'cartpole', 1), ('c_humanoid_CMU', 'humanoid_CMU', 1)):
    p = physics.Physics.from_xml_string(common.read_model(model + '.xml'), batch_size=batch)
    out[leg] = median(p.forward, lambda: p.data.xanchor)
    p.free()
  print(json.dumps(out))


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--parent', help='the revision to compare with')
  ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'host_data_timing.json'))
  ap.add_argument('--measure', action='store_true', help='(child) time the checkout at --root')
  ap.add_argument('--root', default=HERE)
  args = ap.parse_args()
  if args.measure:
    return measure(args.root)
  runs = {'parent': [], 'tree': []}
  with tempfile.TemporaryDirectory() as tmp:
    tar = subprocess.run(['git', '-C', HERE, 'archive', args.parent], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(['tar', '-x', '-C', tmp], input=tar, check=True)
    for _ in range(RUNS):
      for tag, root in (('parent', tmp), ('tree', HERE)):
        got = subprocess.run([sys.executable, os.path.abspath(__file__), '--measure', '--root', root], check=True, cwd=root,
                             stdout=subprocess.PIPE, text=True).stdout
        runs[tag].append(json.loads(got.strip().splitlines()[-1]))
  legs = {}
  for leg in runs['tree'][0]:
    us = {tag: [round(1e6 * r[leg], 2) for r in runs[tag]] for tag in runs}
    legs[leg] = dict(us, parent_median=statistics.median(us['parent']), tree_median=statistics.median(us['tree']))
  a, b = legs['a'], legs['b']
  spread = max(a['parent']) - min(a['parent'])
  a['allowed'] = [round(min(a['parent']) - spread, 2), round(max(a['parent']) + spread, 2)]
  a['ok'] = all(a['allowed'][0] <= t <= a['allowed'][1] for t in a['tree'])
  b['ok'] = b['tree_median'] <= b['parent_median']
  rev = subprocess.run(['git', '-C', HERE, 'rev-parse', args.parent], check=True, stdout=subprocess.PIPE, text=True).stdout.strip()
  result = {'parent': rev, 'device': 'fp64 oracle stand-in (tests/oracle_backend.py)', 'unit': 'microseconds', 'runs': RUNS,
            'repetitions': REPS, 'legs': legs}
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write('\n')
  print(json.dumps(legs, indent=1, sort_keys=True))
  if not (a['ok'] and b['ok']):
    raise SystemExit('host time outside the allowed range: a %s, b %s' % (a['ok'], b['ok']))


if __name__ == '__main__':
  main()

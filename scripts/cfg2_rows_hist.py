"""Constraint rows and solver iterations of the headline workload (bench.py config 2: cheetah, 4096 environments, the
200 settle steps, then the 1050 actions of RandomState(1234)), counted by the fp64 oracle on the CPU -- no GPU needed.

Which environments decide a launch's length is a question about the WORKLOAD: scripts/tail_probe.py drives another one
(actions of RandomState(5), drawn anew after 500 steps) and shows launches with a four-contact wave that this one does not
have.  Uses bench.py's own initial_qpos / make_oracles / threaded_rollout; about a minute on 8 cores.

  python scripts/cfg2_rows_hist.py [--envs 4096] [--steps 1050] [--out profiles/cfg2_rows_hist.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=bench.CONFIGS[2]['batch'])
  ap.add_argument('--steps', type=int, default=1050)      # bench.py config 2: 50 warm-up + 1000 timed launches
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  cfg = bench.CONFIGS[2]
  model = bench.load_model(cfg['asset'])
  B, T, nsub = args.envs, args.steps, cfg['nsub']
  nthreads = bench.host_threads()
  phys = bench.make_oracles(model, bench.initial_qpos(cfg, model, B, 0))
  bench.threaded_rollout(phys, np.zeros((200, B, model.nu)), 1, nthreads)      # Cheetah.initialize_episode's settle steps
  acts = np.random.RandomState(1234).uniform(-1, 1, (T, B, model.nu)).astype(np.float32)
  nefc, iters = {}, {}
  for t in range(T):
    # (a legacy step ends with the position stage of the NEXT step: its rows are those the next launch opens with)
    n = np.array([p.nefc for p in phys])
    bench.threaded_rollout(phys, acts[t:t + 1], nsub, nthreads)
    it = np.array([p.solver_iter for p in phys])
    for hist, v in ((nefc, n), (iters, it)):
      for k, c in zip(*np.unique(v, return_counts=True)):
        hist[int(k)] = hist.get(int(k), 0) + int(c)
  total = B * T
  out = dict(config=2, asset=cfg['asset'], envs=B, steps=T, env_steps=total,
             nefc={str(k): nefc[k] for k in sorted(nefc)}, max_nefc=max(nefc),
             solver_iter={str(k): iters[k] for k in sorted(iters)},
             solver_iter_share={str(k): iters[k] / total for k in sorted(iters)})
  print(json.dumps(out))
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(out, f, indent=1)
      f.write('\n')


if __name__ == '__main__':
  main()

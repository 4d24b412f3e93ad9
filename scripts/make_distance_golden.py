"""Writes tests/golden/distance_cases.npz -- the states of tests/distance_cases.py with the fp64 twin's distance, witness
points, uniqueness flags and own error bound for all 55 pairs -- and profiles/distance_accuracy.json: the twin's worst
error against the closed forms (e_twin) and the worst error of the fp64 / fp32 host builds of csrc/dist_core.h against
the twin.  Needs scipy (the twin); the GPU tests read the fixture instead.

  python scripts/make_distance_golden.py            # fixture + accuracy record
  python scripts/make_distance_golden.py --seeds    # prints the SEEDS table of tests/distance_cases.py (see its docstring)
"""
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import dist_emu_lib as emu      # noqa: E402  pylint: disable=wrong-import-position
import dist_twin as tw      # noqa: E402  pylint: disable=wrong-import-position
import distance_cases as dc      # noqa: E402  pylint: disable=wrong-import-position


def _state_cases(args):
  pos, quat = args
  G = dc.geoms_of(pos, quat)
  out = [dc.twin_case(G, p) for p in dc.PAIRS]
  cf = [None if tw.PLANE in dc.type_pair(p) else tw.closed_form(G[p[0]], G[p[1]]) for p in dc.PAIRS]
  return out, cf


def choose_seeds(tries=50):
  seeds = []
  for k in range(dc.NSTATE):
    for j in range(tries):
      seed = 1000 + k + 100*j
      G = dc.geoms_of(*dc.random_state(k, seed))
      g1, g2 = [G[p[0]] for p in dc.PAIRS], [G[p[1]] for p in dc.PAIRS]
      if not any(emu.pairs(prec, g1, g2, dc.DISTMAX, dc.TOLERANCE, dc.ITERATIONS)['status'].any() for prec in (64, 32)):
        break
    else:
      raise SystemExit('state %d: no seed converges' % k)
    seeds.append(seed)
  return tuple(seeds)


def main():
  if '--seeds' in sys.argv:
    print('SEEDS =', choose_seeds())
    return
  pos, quat, aligned = dc.states()
  with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
    res = pool.map(_state_cases, list(zip(pos, quat)), chunksize=1)
  S, P = len(pos), len(dc.PAIRS)
  dist, fromto = np.zeros((S, P)), np.zeros((S, P, 6))
  unique, gap = np.zeros((S, P), bool), np.zeros((S, P))
  e_twin, n_cf = 0.0, 0
  for s, (cases, cf) in enumerate(res):
    for pi, (d, ft, u, g) in enumerate(cases):
      dist[s, pi], fromto[s, pi], gap[s, pi] = d, ft, g
      unique[s, pi] = u and not aligned[s]
      if cf[pi] is not None:
        e_twin, n_cf = max(e_twin, abs(cf[pi] - d)/max(1.0, abs(d))), n_cf + 1
  e_twin = max(e_twin, float(gap.max()))      # and the twin's own primal-dual gap where the geoms are apart
  os.makedirs(os.path.dirname(dc.GOLDEN), exist_ok=True)
  np.savez_compressed(dc.GOLDEN, pos=pos, quat=quat, aligned=aligned, dist=dist, fromto=fromto, unique=unique, gap=gap)
  # the host builds against the twin
  record = dict(cases=int(S*P), closed_form_cases=int(n_cf), e_twin=e_twin, tolerance=dc.TOLERANCE, iterations=dc.ITERATIONS, caps=emu.caps())
  for prec in (64, 32):
    worst, worst_exact, nstatus, nepa = 0.0, 0.0, 0, 0
    for s in range(S):
      G = dc.geoms_of(pos[s], quat[s])
      r = emu.pairs(prec, [G[p[0]] for p in dc.PAIRS], [G[p[1]] for p in dc.PAIRS], dc.DISTMAX, dc.TOLERANCE, dc.ITERATIONS)
      nstatus, nepa = nstatus + int((r['status'] != 0).sum()), nepa + int(r['epa'].sum())
      ref = np.minimum(dist[s], dc.DISTMAX)
      err = np.abs(r['dist'] - ref)/np.maximum(1.0, np.abs(ref))
      ex = np.array([dc.exact_pair(p) for p in dc.PAIRS])
      worst, worst_exact = max(worst, float(err.max())), max(worst_exact, float(err[ex].max()))
    record['host_f%d' % prec] = dict(worst_rel_error=worst, worst_rel_error_exact_pairs=worst_exact, status_nonzero=nstatus, epa_cases=nepa)
  with open(os.path.join(ROOT, 'profiles', 'distance_accuracy.json'), 'w') as f:
    json.dump(record, f, indent=1, sort_keys=True)
    f.write('\n')
  print(json.dumps(record, indent=1, sort_keys=True))
  print('wrote', dc.GOLDEN, os.path.getsize(dc.GOLDEN), 'bytes')


if __name__ == '__main__':
  main()

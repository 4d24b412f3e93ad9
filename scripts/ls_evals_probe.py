"""Line-search cost evaluations and passes per search (a fused pass of the bracket phase evaluates several points and
counts once) and Newton iterations per step of the emulated kernel core under the bench workloads -- the emulation runs
the same algorithm as the device, so the counts are the device's.  Config 2 (cheetah) as the benchmark runs it: its start
states, 200 settle steps (not counted), then random actions; by Newton iterations of the env-step as well, since a launch
waits for the environment with the most."""
import collections
import os
import sys, ctypes, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bench
from emu_lib import EmuPhysics, lib
from dm_control_amd.suite import common
L = lib(os.path.join(ROOT, 'tests', 'emu', 'ls_fused.cpp'), 'emu_ls_probe')
def counts():
  out = (ctypes.c_longlong*6)(); ps = (ctypes.c_longlong*3)()
  L.emu_ls_counts_get(out); L.emu_ls_passes_get(ps)
  return np.array(list(out) + list(ps))      # [6]: passes, [7]: searches in the bracket phase, [8]: fused passes
for prec in (64, 32):
 for cid in (2, 5, 4):
  cfg = bench.CONFIGS[cid]
  m = bench.load_model(cfg['asset'])
  caps = {k: v for k, v in common.DEFAULT_CAPS.get(cfg['asset'], {}).items() if k in ('nconmax','njmax','njcon')}
  rs = np.random.RandomState(1234 if cid == 2 else 0)
  iters = 0; steps = 0
  out = np.zeros(9, np.int64)
  by_iter = collections.defaultdict(lambda: np.zeros(10, np.int64))
  nenv = 16 if cid == 2 else 2
  q0 = bench.initial_qpos(cfg, m, nenv, 0)
  for env in range(nenv):
    e = EmuPhysics(m, prec, **caps)
    e.qpos[:] = q0[env]
    if cid == 2:
      e.step(200)
    for t in range(250 if cid == 2 else 30):
      e.ctrl[:] = rs.uniform(-1,1,m.nu)
      for k in range(cfg['nsub']):
        b = counts(); e.step(1); d = counts() - b
        it = int(e.solver_iter[0]); iters += it; steps += 1
        out += d; by_iter[it][:9] += d; by_iter[it][9] += 1
  print('prec', prec, 'config', cid, 'ls calls per step %.2f' % (out[0]/steps), 'evals per ls %.2f' % (out[1]/max(1,out[0])),
        'passes per ls %.2f' % (out[6]/max(1,out[0])), 'searches in the bracket phase %.1f %%' % (100.0*out[7]/max(1,out[0])), 'iters/step %.2f' % (iters/steps),
        'noslip sweeps per pass %.2f' % (out[3]/max(1,out[2])), 'qcqp iterations per call %.2f (%.1f calls per step)' % (out[5]/max(1,out[4]), out[4]/steps))
  if cid == 2:
    for it in sorted(by_iter):
      v = by_iter[it]
      print('   %d Newton iterations: %5.2f %% of env-steps, evaluations per env-step %.2f, passes %.2f' % (it, 100.0*v[9]/steps, v[1]/v[9], v[6]/v[9]))

"""The register-resident Newton solve of the small dense models (step_core.h primal_solve_regs) against the LDS solve it
replaces: the same sources built with -DDMC_NO_NEWTON_REGS as an on-demand plugin (dm_control_amd/specialise.py).

fp64: every sum of the register solve keeps the order of the LDS path (no sum had to change order), so the two kernels
must agree bit for bit -- qpos, qvel, sensordata, solver_iter and the warnings -- over 240 steps of a seeded batch, for
cheetah, walker and hopper and for a small model whose environments cross the cap of 16 constraint rows in both
directions, so that the fallback to the LDS solve and waves whose two environments take different paths are exercised.
The fp64 kernels of the library do not instantiate the register solve (they sit at the 256-VGPR cap and would gain
private segment, DESIGN.md section 4: DMC_NEWTON_REGS_F64_NV is 0), so the fp64 register solve is a plugin built with
-DDMC_NEWTON_REGS_F64_NV=16; it is compared with the LDS plugin AND with the library's default kernel.

fp32 is compiled with contraction on, so there the order of a sum is not the whole story: which products are fused into
their sum is the compiler's choice and differs between the two shapes of the code unless it is spelt out.  The register
solve spells it out where the LDS path's choice is not the obvious one (nr_dot, nr_jtf and the updates in step_core.h), and
the two fp32 kernels must then agree bit for bit as well -- the models are chaotic, a last-bit difference in one solve is
another trajectory a few hundred steps later, and the benchmark's end state would no longer be the one the LDS solve gives.

fp32 also: the one-step teacher-forced error against the fp64 oracle stays within test_gpu_parity.TOL_F32_ONE_STEP for both
paths, and the mean solver_iter of the two paths differs by no more than two fp32 builds of these sources differ today:
the committed fp32 measurements of config 2 (DESIGN.md sections 2 and 4, other lane widths / operation orders of the same
solver) report 1.326, 1.33 and 1.34 iterations per step, a spread of 0.014 -- the bound is 0.02 iterations per step."""
import os

import numpy as np
import pytest

from dm_control_amd import mjcf_compiler as mc
from dm_control_amd.suite import common

pytestmark = pytest.mark.gpu

LDS_FLAGS = '-DDMC_NO_NEWTON_REGS'
F64_REGS_FLAGS = '-DDMC_NEWTON_REGS_F64_NV=16'
ITER_SPREAD = 0.02
BAKED = ['cheetah', 'walker', 'hopper']

# Planar chain of four capsules (6 dofs, hinge limits, pyramidal contacts: one-sided rows only).  A capsule lying on the
# floor has two contacts of four rows each, so an environment at rest on the ground has more than 16 rows, one in the air
# only its active joint limits: environments dropped from different heights cross the cap at different steps.
CHAIN = """
<mujoco>
  <option timestep="0.004"/>
  <worldbody>
    <geom name="floor" type="plane" size="5 5 .1"/>
    <body name="b0" pos="0 0 .1">
      <joint name="x" type="slide" axis="1 0 0"/><joint name="z" type="slide" axis="0 0 1"/><joint name="tilt" type="hinge" axis="0 1 0"/>
      <geom type="capsule" fromto="-.2 0 0 .2 0 0" size=".05" mass="2"/>
      <body name="b1" pos=".2 0 0">
        <joint name="j1" type="hinge" axis="0 1 0" range="-50 50" limited="true" damping=".1"/>
        <geom type="capsule" fromto=".06 0 0 .4 0 0" size=".05" mass="1"/>
        <body name="b2" pos=".4 0 0">
          <joint name="j2" type="hinge" axis="0 1 0" range="-50 50" limited="true" damping=".1"/>
          <geom type="capsule" fromto=".06 0 0 .4 0 0" size=".05" mass="1"/>
          <body name="b3" pos=".4 0 0">
            <joint name="j3" type="hinge" axis="0 1 0" range="-50 50" limited="true" damping=".1"/>
            <geom type="capsule" fromto=".06 0 0 .4 0 0" size=".05" mass="1"/>
          </body>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator><motor joint="j1" gear="20"/><motor joint="j2" gear="20"/><motor joint="j3" gear="20"/></actuator>
  <sensor><jointpos joint="j1"/><jointvel joint="j3"/><subtreelinvel body="b0"/></sensor>
</mujoco>
"""


def _model(name):
  return mc.compile_xml(CHAIN if name == 'chain' else common.read_model(name + '.xml'))


def _init(m, name, B, seed):
  rs = np.random.RandomState(seed)
  q = np.tile(m.qpos0, (B, 1))
  if name == 'chain':
    q[:, 1] = rs.uniform(0.0, 1.2, B)      # drop height: the environments land at different steps
    q[:, 3:] += rs.uniform(-.5, .5, (B, m.nq - 3))
  else:
    lim = m.jnt_limited == 1
    lo, hi = m.jnt_range[lim].T
    q[:, lim] = rs.uniform(lo, hi, (B, int(lim.sum())))
  return q


def _plugin(monkeypatch, m, B, precision, flags):
  """A batch on the on-demand specialised kernel of these sources built with `flags` (the baked kernel hidden)."""
  from dm_control_amd.batch import BatchedPhysics
  monkeypatch.setenv('DMC_NO_STATIC', '1')
  monkeypatch.setenv('DMC_SPEC_FLAGS', flags)
  b = BatchedPhysics(m, B, precision=precision, specialise='build')
  monkeypatch.delenv('DMC_NO_STATIC')
  monkeypatch.delenv('DMC_SPEC_FLAGS')
  assert b.specialised == 'attached' and b.info()['static_id'] == 1000, b.info()
  return b


def _default(monkeypatch, m, name, B, precision):
  """The kernel a user gets: the baked one of a suite model, the plain plugin for the chain."""
  from dm_control_amd.batch import BatchedPhysics
  for v in ('DMC_SPEC_PLUGIN', 'DMC_SPEC_FLAGS', 'DMC_NO_STATIC'):
    monkeypatch.delenv(v, raising=False)
  if name in BAKED:
    b = BatchedPhysics(m, B, precision=precision)
    assert 0 <= b.info()['static_id'] < 1000, b.info()
    return b
  return _plugin(monkeypatch, m, B, precision, '')


def _pair(monkeypatch, m, name, B, precision):
  """fp32 (register solve, LDS solve): the default kernel and the plugin of the same sources with the LDS solve."""
  regs = _default(monkeypatch, m, name, B, precision)
  lds = _plugin(monkeypatch, m, B, precision, LDS_FLAGS)
  assert lds.info()['lanes_per_env'] == regs.info()['lanes_per_env']
  return regs, lds


@pytest.mark.parametrize('name', BAKED + ['chain'])
def test_fp64_register_solve_is_bit_identical_to_the_lds_solve(monkeypatch, name):
  m = _model(name)
  B, T = 128, 240
  dflt = _default(monkeypatch, m, name, B, 64)
  regs = _plugin(monkeypatch, m, B, 64, F64_REGS_FLAGS)
  lds = _plugin(monkeypatch, m, B, 64, LDS_FLAGS)
  assert lds.info()['lanes_per_env'] == regs.info()['lanes_per_env'] == dflt.info()['lanes_per_env']
  q = _init(m, name, B, 1)
  rs = np.random.RandomState(2)
  for b in (dflt, regs, lds):
    b.set('qpos', q)
  rows_lo = rows_hi = mixed = 0
  iters = 0
  for t in range(T):
    a = rs.uniform(-1, 1, (B, m.nu))
    for b in (dflt, regs, lds):
      b.set_control(a)
      b.step()
    if t % 8 == 7 or t == T - 1:
      for f in ('qpos', 'qvel', 'sensordata', 'solver_iter', 'warning'):
        np.testing.assert_array_equal(regs.get(f), lds.get(f), err_msg='%s: %s at step %d' % (name, f, t))
        np.testing.assert_array_equal(dflt.get(f), lds.get(f), err_msg='%s (default kernel): %s at step %d' % (name, f, t))
    n = regs.get('nefc')[:, 0]
    rows_lo += int(((n > 0) & (n <= 16)).sum()); rows_hi += int((n > 16).sum())
    lpe = regs.info()['lanes_per_env']
    if lpe == 32:      # two environments per wave: neighbours
      mixed += int(((n[0::2] > 16) != (n[1::2] > 16)).sum())
    iters += int(regs.get('solver_iter').sum())
  print('measured: %s fp64 bit-identical over %d steps x %d envs; solves with 1..16 rows %d, with more %d, waves with one '
        'environment on each path %d, Newton iterations %d' % (name, T, B, rows_lo, rows_hi, mixed, iters))
  assert rows_lo > 0 and iters > 0      # the register solve ran
  if name == 'chain':
    assert rows_hi > 0 and mixed > 0      # ... and so did the fallback, in the same wave
  assert np.isfinite(regs.get('qpos')).all()
  dflt.close(); regs.close(); lds.close()


@pytest.mark.parametrize('name', BAKED + ['chain'])
def test_fp32_register_solve_is_bit_identical_to_the_lds_solve(monkeypatch, name):
  """The suite models: every environment, bit for bit (what keeps the benchmark's end state the LDS solve's).  The chain
  drives environments over the cap, and such an environment runs the LDS source in BOTH builds -- two compilations of the same
  text, whose fp32 contraction is the compiler's choice per function body (the 6-dof plugin's fallback fuses the last
  column pair of the Hessian's assembly, the LDS-only build adds it: seen in the ISA, nothing the register solve decides).
  So the chain's claim is the register solve's: an environment is compared for as long as every one of its solves so far
  had at most 16 rows."""
  m = _model(name)
  B, T = 128, 240
  regs, lds = _pair(monkeypatch, m, name, B, 32)
  q = _init(m, name, B, 1)
  rs = np.random.RandomState(2)
  for b in (regs, lds):
    b.set('qpos', q)
  fields = ('qpos', 'qvel', 'sensordata', 'solver_iter', 'warning')
  clean = np.ones(B, bool)      # chain: no solve of the environment has left the register path yet
  first, solves = None, 0
  for t in range(T):
    a = rs.uniform(-1, 1, (B, m.nu))
    for b in (regs, lds):
      b.set_control(a)
      b.step()
    n = regs.get('nefc')[:, 0]
    if name == 'chain':
      clean &= (n <= 16) & (lds.get('nefc')[:, 0] <= 16)
    solves += int(((n > 0) & clean).sum())
    if first is None and not all(np.array_equal(regs.get(f)[clean], lds.get(f)[clean]) for f in fields):
      first = t
  print('measured: %s fp32 regs against lds over %d steps x %d envs: first step that differs %s; compared to the end %d '
        'environments, register solves among the compared %d' % (name, T, B, first, int(clean.sum()), solves))
  assert first is None, '%s: first difference at step %d' % (name, first)
  assert solves > 0
  assert np.isfinite(regs.get('qpos')).all()
  regs.close(); lds.close()


@pytest.mark.parametrize('name', BAKED)
def test_fp32_one_step_error_and_iteration_count_of_both_paths(monkeypatch, name):
  import test_gpu_parity as parity
  from oracle import oracle
  m = _model(name)
  # one-step teacher-forced error against the fp64 oracle, both paths (the tolerance of tests/test_gpu_parity.py)
  NE, T = 32, 100
  q = _init(m, name, NE, 3)
  refs = parity._oracles(m, q)
  oracle.rollout_legacy(refs, np.zeros((100, NE, m.nu)))
  regs, lds = _pair(monkeypatch, m, name, NE, 32)
  rs = np.random.RandomState(9)
  worst = {'regs': 0.0, 'lds': 0.0}
  for t in range(T):
    a = rs.uniform(-1, 1, (NE, m.nu))
    for key, b in (('regs', regs), ('lds', lds)):
      b.set('qpos', np.stack([p.qpos for p in refs]))
      b.set('qvel', np.stack([p.qvel for p in refs]))
      b.set('qacc_warmstart', np.stack([p.qacc_warmstart for p in refs]))
      b.set_control(a)
      b.step()
    oracle.rollout_legacy(refs, a[None])
    qo = np.stack([p.qpos for p in refs])
    for key, b in (('regs', regs), ('lds', lds)):
      worst[key] = max(worst[key], parity._rel_err(b.get('qpos'), qo))
  regs.close(); lds.close()
  # mean solver_iter of the two paths, open loop from the same seeded batch
  B, T2 = 1024, 200
  regs, lds = _pair(monkeypatch, m, name, B, 32)
  q = _init(m, name, B, 4)
  for b in (regs, lds):
    b.set('qpos', q)
  tot = {'regs': 0, 'lds': 0}
  for t in range(T2):
    a = rs.uniform(-1, 1, (B, m.nu))
    for key, b in (('regs', regs), ('lds', lds)):
      b.set_control(a)
      b.step()
      tot[key] += int(b.get('solver_iter').sum())
  mean = {k: v / float(B * T2) for k, v in tot.items()}
  same = bool(np.array_equal(regs.get('qpos'), lds.get('qpos')))
  print('measured: %s fp32 one-step rel qpos error regs %.3g lds %.3g (tolerance %.1g); mean solver_iter regs %.4f lds %.4f; '
        'end state bit-identical: %s' % (name, worst['regs'], worst['lds'], parity.TOL_F32_ONE_STEP, mean['regs'], mean['lds'], same))
  assert not regs.get('warning').any() and not lds.get('warning').any()
  regs.close(); lds.close()
  assert worst['regs'] < parity.TOL_F32_ONE_STEP, worst
  assert worst['lds'] < parity.TOL_F32_ONE_STEP, worst
  assert abs(mean['regs'] - mean['lds']) <= ITER_SPREAD, mean

"""The register section of the acceleration stage of the small dense models (step_core.h primal_solve_regs<N, true>:
qfrc_smooth, qacc_smooth, the warm start's choice, the Newton solve and mj_Euler's damped solve without a trip through
LDS) against the code it replaces: the same sources built with -DDMC_NO_ACC_REGS as an on-demand plugin, built like the
plugins of tests/test_gpu_newton_regs.py, whose models, seeds and helpers these tests share.

Every sum of the section keeps the order and, in fp32, the fusing of the LDS code, so the two kernels must agree bit for
bit -- qpos, qvel, qacc, qacc_warmstart, sensordata, solver_iter and the warnings.  fp64 (the register section is opt-in
there: -DDMC_NEWTON_REGS_F64_NV=16 on both sides) and fp32 (the default kernel), over 240 steps; a batch whose last wave
holds one environment; and the launches in which mj_Euler's damped solve must NOT be taken from the acceleration stage
(RK4, mjDSBL_EULERDAMP, mj_forward before a step) or must be taken anew in every pass (a launch of three steps).

The four-capsule chain drives environments through all three classes -- no constraint row (in the air, hinges inside
their limits: the register section now takes these too), 1 .. 16 rows, and more than 16 rows (the LDS code, per
environment, also beside a neighbour of the same wave that stays in registers); the counts are read back from nefc."""
import numpy as np
import pytest

from dm_control_amd import mjcf_compiler as mc

import test_gpu_newton_regs as nrt

pytestmark = pytest.mark.gpu

LDS_FLAGS = '-DDMC_NO_ACC_REGS'
F64_FLAGS = '-DDMC_NEWTON_REGS_F64_NV=16'
FIELDS = ('qpos', 'qvel', 'qacc', 'qacc_warmstart', 'sensordata', 'solver_iter', 'warning')
MODELS = ['cheetah', 'hopper', 'chain']
EULERDAMP = mc.C['DMC_DSBL_EULERDAMP']


def _classes(n, lpe):
  """Per-step counts of environments without rows, with 1 .. 16, with more, and of waves whose two environments differ."""
  mixed = int(((n[0::2] > 16) != (n[1::2] > 16)).sum()) if lpe == 32 and len(n) % 2 == 0 else 0
  return np.array([int((n == 0).sum()), int(((n > 0) & (n <= 16)).sum()), int((n > 16).sum()), mixed])


# the chain with the sensors whose evaluation (rne_post_constraint) writes body accelerations and forces over the memory
# of the solver's vectors, where the acceleration stage leaves mj_Euler's damped solve
CHAIN_IMU = nrt.CHAIN.replace('<geom type="capsule" fromto=".06 0 0 .4 0 0" size=".05" mass="1"/>',
                              '<geom type="capsule" fromto=".06 0 0 .4 0 0" size=".05" mass="1"/><site name="imu" pos=".2 0 0"/>', 1)
CHAIN_IMU = CHAIN_IMU.replace('<sensor>', '<sensor><accelerometer site="imu"/><force site="imu"/><torque site="imu"/>')
assert CHAIN_IMU.count('site="imu"') == 3 and CHAIN_IMU.count('<site') == 1


def _default(monkeypatch, m, name, B):
  """fp32, the kernel a user gets: the baked one of a suite model, the plain plugin for a model of this file."""
  from dm_control_amd.batch import BatchedPhysics
  if name.startswith('chain'):
    return nrt._plugin(monkeypatch, m, B, 32, '')
  for v in ('DMC_SPEC_PLUGIN', 'DMC_SPEC_FLAGS', 'DMC_NO_STATIC'):
    monkeypatch.delenv(v, raising=False)
  b = BatchedPhysics(m, B, precision=32)
  assert 0 <= b.info()['static_id'] < 1000, '%s has no baked kernel: %s' % (name, b.info())
  return b


def _same(a, b, sel=slice(None)):
  return [f for f in FIELDS if not np.array_equal(a.get(f)[sel], b.get(f)[sel])]


@pytest.mark.parametrize('name', MODELS)
def test_fp64_register_section_is_bit_identical_to_the_lds_stage(monkeypatch, name):
  m = nrt._model(name)
  B, T = 128, 240
  regs = nrt._plugin(monkeypatch, m, B, 64, F64_FLAGS)
  lds = nrt._plugin(monkeypatch, m, B, 64, F64_FLAGS + ' ' + LDS_FLAGS)
  lpe = regs.info()['lanes_per_env']
  assert lds.info()['lanes_per_env'] == lpe
  q = nrt._init(m, name, B, 1)
  rs = np.random.RandomState(2)
  for b in (regs, lds):
    b.set('qpos', q)
  count = np.zeros(4, int)
  for t in range(T):
    a = rs.uniform(-1, 1, (B, m.nu))
    for b in (regs, lds):
      b.set_control(a)
      b.step()
    if t % 8 == 7 or t == T - 1:
      assert not _same(regs, lds), '%s: %s at step %d' % (name, _same(regs, lds), t)
    count += _classes(regs.get('nefc')[:, 0], lpe)
  print('measured: %s fp64 bit-identical over %d steps x %d envs; env-steps without rows %d, with 1..16 rows %d, with more %d, '
        'waves with one environment on each path %d' % ((name, T, B) + tuple(count)))
  assert count[1] > 0
  if name == 'chain':
    assert (count > 0).all(), count      # every class, and both paths in one wave
  assert np.isfinite(regs.get('qpos')).all()
  regs.close(); lds.close()


@pytest.mark.parametrize('name', MODELS)
def test_fp32_register_section_is_bit_identical_to_the_lds_stage(monkeypatch, name):
  """The chain is compared as tests/test_gpu_newton_regs.py compares it, and for its reason: an environment with more than
  16 rows runs the LDS source in both builds, two compilations whose fp32 contraction is the compiler's choice per function
  body, so an environment is compared for as long as every one of its passes so far stayed on the register path."""
  m = nrt._model(name)
  B, T = 128, 240
  regs = _default(monkeypatch, m, name, B)
  lds = nrt._plugin(monkeypatch, m, B, 32, LDS_FLAGS)
  lpe = regs.info()['lanes_per_env']
  assert lds.info()['lanes_per_env'] == lpe
  q = nrt._init(m, name, B, 1)
  rs = np.random.RandomState(2)
  for b in (regs, lds):
    b.set('qpos', q)
  clean = np.ones(B, bool)
  first = None
  count = np.zeros(4, int)
  compared = np.zeros(2, int)      # env-steps compared: without rows, with 1 .. 16
  for t in range(T):
    a = rs.uniform(-1, 1, (B, m.nu))
    for b in (regs, lds):
      b.set_control(a)
      b.step()
    n = regs.get('nefc')[:, 0]
    if name == 'chain':
      clean &= (n <= 16) & (lds.get('nefc')[:, 0] <= 16)
    count += _classes(n, lpe)
    compared += [int(((n == 0) & clean).sum()), int(((n > 0) & clean).sum())]
    if first is None and _same(regs, lds, clean):
      first = (t, _same(regs, lds, clean))
  print('measured: %s fp32 register section against the LDS stage over %d steps x %d envs: first step that differs %s; compared '
        'to the end %d environments; compared env-steps without rows %d, with 1..16 rows %d; all env-steps without rows %d, with '
        '1..16 %d, with more %d, waves with one environment on each path %d'
        % ((name, T, B, first, int(clean.sum())) + tuple(compared) + tuple(count)))
  assert first is None, '%s: first difference at step %d in %s' % ((name,) + first)
  assert compared[1] > 0
  if name == 'chain':
    assert (count > 0).all() and (compared > 0).all(), (count, compared)
  assert np.isfinite(regs.get('qpos')).all()
  regs.close(); lds.close()


def test_fp32_ragged_batch_whose_last_wave_holds_one_environment(monkeypatch):
  m = nrt._model('cheetah')
  B, T = 41, 60
  regs = _default(monkeypatch, m, 'cheetah', B)
  lds = nrt._plugin(monkeypatch, m, B, 32, LDS_FLAGS)
  assert regs.info()['lanes_per_env'] == lds.info()['lanes_per_env'] == 32
  q = nrt._init(m, 'cheetah', B, 5)
  rs = np.random.RandomState(6)
  for b in (regs, lds):
    b.set('qpos', q)
  for t in range(T):
    a = rs.uniform(-1, 1, (B, m.nu))
    for b in (regs, lds):
      b.set_control(a)
      b.step()
    assert not _same(regs, lds), 'step %d: %s' % (t, _same(regs, lds))
  assert regs.get('solver_iter').sum() > 0 and np.isfinite(regs.get('qpos')).all()
  regs.close(); lds.close()


@pytest.mark.parametrize('variant', ['rk4', 'eulerdamp_disabled', 'forward_then_step', 'three_steps_per_launch'])
def test_fp32_launches_that_must_not_reuse_a_damped_solve(monkeypatch, variant):
  """rk4: cartpole, whose stages integrate without mj_Euler.  eulerdamp_disabled: mj_Euler takes qacc as it is.
  forward_then_step: mj_forward's acceleration stage is followed by no integration, the step after it by one.
  three_steps_per_launch: acceleration stage -> mj_Euler three times in one launch, the mark set and consumed each time."""
  name = 'cartpole' if variant == 'rk4' else 'cheetah'
  m = nrt._model(name)
  B, T = 128, 60
  regs = _default(monkeypatch, m, name, B)
  lds = nrt._plugin(monkeypatch, m, B, 32, LDS_FLAGS)
  assert regs.info()['lanes_per_env'] == lds.info()['lanes_per_env']
  rs = np.random.RandomState(7)
  if name == 'cartpole':
    q = np.tile(m.qpos0, (B, 1)) + rs.uniform(-1, 1, (B, m.nq))
  else:
    q = nrt._init(m, name, B, 8)
  for b in (regs, lds):
    b.set('qpos', q)
    if variant == 'eulerdamp_disabled':
      b.set_opt('disableflags', EULERDAMP)
  for t in range(T):
    a = rs.uniform(-1, 1, (B, m.nu))
    for b in (regs, lds):
      b.set_control(a)
      if variant == 'forward_then_step':
        b.forward()
      b.step(3 if variant == 'three_steps_per_launch' else 1)
    assert not _same(regs, lds), '%s step %d: %s' % (variant, t, _same(regs, lds))
  assert np.isfinite(regs.get('qpos')).all() and np.abs(regs.get('qvel')).max() > 0
  regs.close(); lds.close()


@pytest.mark.parametrize('precision', [32, 64])
def test_acceleration_sensors_do_not_cost_the_damped_solve(monkeypatch, precision):
  """A damped Euler model with an accelerometer, a force and a torque sensor, single-step launches: every launch evaluates
  the sensors between the acceleration stage and mj_Euler, over the memory that held the stage's damped solve."""
  m = mc.compile_xml(CHAIN_IMU)
  B, T = 128, 120
  if precision == 64:
    regs = nrt._plugin(monkeypatch, m, B, 64, F64_FLAGS)
    lds = nrt._plugin(monkeypatch, m, B, 64, F64_FLAGS + ' ' + LDS_FLAGS)
  else:
    regs = _default(monkeypatch, m, 'chain_imu', B)
    lds = nrt._plugin(monkeypatch, m, B, 32, LDS_FLAGS)
  q = nrt._init(m, 'chain', B, 1)
  rs = np.random.RandomState(2)
  for b in (regs, lds):
    b.set('qpos', q)
  clean = np.ones(B, bool)      # (fp32: as in the chain's comparison above)
  compared = 0
  for t in range(T):
    a = rs.uniform(-1, 1, (B, m.nu))
    for b in (regs, lds):
      b.set_control(a)
      b.step()
    n = regs.get('nefc')[:, 0]
    if precision == 32:
      clean &= (n <= 16) & (lds.get('nefc')[:, 0] <= 16)
    compared += int(clean.sum())
    assert not _same(regs, lds, clean), 'fp%d step %d: %s' % (precision, t, _same(regs, lds, clean))
  assert compared > 0 and np.abs(regs.get('sensordata')[:, :9]).max() > 0 and np.isfinite(regs.get('qpos')).all()
  regs.close(); lds.close()

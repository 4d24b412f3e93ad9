"""The shortened fixed stages of the small models' kernels against the code they replace: this tree's kernel against the
on-demand plugin of the same sources built with -DDMC_NO_CONTENT_DIMS -DDMC_NO_ROW_REDUCE (every joint and sensor type
assumed present; the reductions of the register section over all 32 lanes of the group), built like the plugins of
tests/test_gpu_newton_regs.py, whose models, seeds and helpers these tests share.

Neither switch changes an operand or the order of a sum: the content facts remove branches that are never taken, and the
16-lane reductions leave out the addition of the other row's exact zero.  So the two kernels must agree bit for bit --
qpos, qvel, qacc, qacc_warmstart, sensordata, solver_iter and the warnings, every 8 steps of 240 -- in fp64 (the register
section is opt-in there: -DDMC_NEWTON_REGS_F64_NV=16 on both sides) and in fp32, for B = 128 and for B = 3, whose last wave
holds a single environment.

Models: cheetah, hopper, the four-capsule chain (environments without rows, with 1 .. 16, with more than 16, and waves
with one environment of each kind; fp32: an environment is compared while all its solves stayed on the register path,
for the reason tests/test_gpu_acc_regs.py gives) and the all-types model of tests/content_dims_models.py (free, ball,
slide and hinge joints, a mocap body, every sensor type; at most 14 rows, so never off the register path)."""
import numpy as np
import pytest

import content_dims_models as cdm
import test_gpu_newton_regs as nrt

pytestmark = pytest.mark.gpu

REF_FLAGS = '-DDMC_NO_CONTENT_DIMS -DDMC_NO_ROW_REDUCE'
F64_FLAGS = '-DDMC_NEWTON_REGS_F64_NV=16'
FIELDS = ('qpos', 'qvel', 'qacc', 'qacc_warmstart', 'sensordata', 'solver_iter', 'warning')
MODELS = ['cheetah', 'hopper', 'chain', 'alltypes']
T = 240


def _model(name):
  return cdm.alltypes() if name == 'alltypes' else nrt._model(name)


def _pair(monkeypatch, m, name, B, precision):
  """(this tree's kernel, the reference plugin).  fp32: the kernel a user gets -- the baked one of a suite model, the plain
  plugin otherwise; fp64: the plugins with the register section switched on."""
  if precision == 64:
    new = nrt._plugin(monkeypatch, m, B, 64, F64_FLAGS)
    ref = nrt._plugin(monkeypatch, m, B, 64, F64_FLAGS + ' ' + REF_FLAGS)
  else:
    new = nrt._default(monkeypatch, m, name, B, 32)
    ref = nrt._plugin(monkeypatch, m, B, 32, REF_FLAGS)
  assert new.info()['lanes_per_env'] == ref.info()['lanes_per_env']
  return new, ref


def _start(m, name, B, batches):
  if name == 'alltypes':
    q, v = cdm.alltypes_init(m, B, 1)
    for b in batches:
      b.set('qpos', q)
      b.set('qvel', v)
  else:
    q = nrt._init(m, name, B, 1)
    for b in batches:
      b.set('qpos', q)


def _differs(a, b, sel):
  return [f for f in FIELDS if not np.array_equal(a.get(f)[sel], b.get(f)[sel])]


def _run(monkeypatch, name, B, precision):
  m = _model(name)
  new, ref = _pair(monkeypatch, m, name, B, precision)
  lpe = new.info()['lanes_per_env']
  _start(m, name, B, (new, ref))
  rs = np.random.RandomState(2)
  clean = np.ones(B, bool)      # fp32 chain: the environments whose solves all stayed on the register path, in both kernels
  count = np.zeros(4, int)      # env-steps without rows, with 1 .. 16, with more; waves with one environment on each path
  compared = 0
  moved = np.zeros(m.nv)
  for t in range(T):
    a = rs.uniform(-1, 1, (B, m.nu))
    for b in (new, ref):
      b.set_control(a)
      b.step()
    n = new.get('nefc')[:, 0]
    if name == 'chain' and precision == 32:
      clean &= (n <= 16) & (ref.get('nefc')[:, 0] <= 16)
    count[:3] += [int((n == 0).sum()), int(((n > 0) & (n <= 16)).sum()), int((n > 16).sum())]
    if lpe == 32 and B % 2 == 0:
      count[3] += int(((n[0::2] > 16) != (n[1::2] > 16)).sum())
    if t % 8 == 7 or t == T - 1:
      bad = _differs(new, ref, clean)
      assert not bad, '%s fp%d B=%d: %s differ at step %d' % (name, precision, B, bad, t)
      compared += int(clean.sum())
      moved = np.maximum(moved, np.abs(new.get('qvel')).max(axis=0))
  print('measured: %s fp%d B=%d bit-identical at every 8th of %d steps; env-steps without rows %d, with 1..16 rows %d, with more '
        '%d, waves with one environment on each path %d; environments compared to the end %d'
        % ((name, precision, B, T) + tuple(count) + (int(clean.sum()),)))
  assert compared > 0 and count[1] > 0
  assert np.isfinite(new.get('qpos')).all()
  if name == 'chain' and B >= 128:
    assert (count > 0).all(), count      # every class, and a mixed wave
    assert clean.any() or precision == 64
  if name == 'alltypes':
    assert count[2] == 0, count           # never more than 16 rows: the register path throughout
    assert (moved[cdm.FREE_DOFS] > 0).all() and (moved[cdm.BALL_DOFS] > 0).all(), moved      # stepped through the free and the ball joint
    assert np.abs(new.get('sensordata')).max() > 0
  new.close(); ref.close()


@pytest.mark.parametrize('name', MODELS)
def test_fp64_is_bit_identical_to_the_reference_build(monkeypatch, name):
  _run(monkeypatch, name, 128, 64)


@pytest.mark.parametrize('name', MODELS)
def test_fp32_is_bit_identical_to_the_reference_build(monkeypatch, name):
  _run(monkeypatch, name, 128, 32)


@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('name', MODELS)
def test_ragged_batch_whose_last_wave_holds_one_environment(monkeypatch, name, precision):
  _run(monkeypatch, name, 3, precision)

"""The cooperative opening stage (csrc/step_kernel.hip.h coop_open_phase: the two sides of the opening stage on the two
waves of a pair, 16 lanes per environment) on the device against the stage as one wave runs it at 32 lanes: the same
sources built with -DDMC_NO_COOP_OPEN as an on-demand plugin (dm_control_amd/specialise.py), against the default kernel.

Per item the arithmetic is the same text; only which wave and which lane evaluates an item changes.  So the two kernels
must agree bit for bit -- state, sensors, ncon, nefc, solver_iter and every warning row after every launch -- in fp32, and
in fp64 (plugins with the register solve on both sides, which is what gives an fp64 kernel the cooperative stage).

Small batches get one-wave workgroups, which never cooperate: DMC_WAVES=4 around the batch's construction forces four-wave
workgroups.  The batch sizes then cover a pair with an empty partner wave (1, 2), a ragged wave (1, 3, 5), a workgroup of
which three waves have no item (1, 2), two workgroups of which one is partial (9) and three (23)."""
import numpy as np
import pytest

import test_gpu_newton_regs as nr

pytestmark = pytest.mark.gpu

SOLO_FLAGS = '-DDMC_NO_COOP_OPEN'
FIELDS = ('qpos', 'qvel', 'qacc_warmstart', 'time', 'sensordata', 'ncon', 'nefc', 'solver_iter', 'warning')
T = 40
BADQPOS, BADQVEL, BADQACC = 4, 5, 6      # include/dmc_model_layout.h: DMC_WARN_*


def _pair(monkeypatch, name, B, precision=32, waves=4):
  """(default kernel, the same sources without the cooperative stage), both on workgroups of `waves` waves (0: the
  library's choice)."""
  m = nr._model(name)
  if waves:
    monkeypatch.setenv('DMC_WAVES', str(waves))
  if precision == 32:
    coop = nr._default(monkeypatch, m, name, B, 32)
    solo = nr._plugin(monkeypatch, m, B, 32, SOLO_FLAGS)
  else:
    coop = nr._plugin(monkeypatch, m, B, 64, nr.F64_REGS_FLAGS)
    solo = nr._plugin(monkeypatch, m, B, 64, nr.F64_REGS_FLAGS + ' ' + SOLO_FLAGS)
  monkeypatch.delenv('DMC_WAVES', raising=False)
  for k in ('lanes_per_env', 'waves_per_block', 'grid', 'work_queue'):
    assert coop.info()[k] == solo.info()[k], (k, coop.info(), solo.info())
  assert coop.info()['lanes_per_env'] == 32 and coop.info()['work_queue'] == 0
  if waves:
    assert coop.info()['waves_per_block'] == waves
  assert solo.info()['launch']['coop_open'] == 0
  q = nr._init(m, name, B, 1)
  for b in (coop, solo):
    b.set('qpos', q)
  return m, coop, solo


def _same(coop, solo, where):
  for f in FIELDS:
    x, y = coop.get(f), solo.get(f)
    assert np.array_equal(x, y, equal_nan=(x.dtype.kind == 'f')), (where, f, np.argwhere(x != y)[:4])


def _run(m, coop, solo, launch, between=None, steps=T, seed=2):
  rs = np.random.RandomState(seed)
  rows = solves = 0
  for t in range(steps):
    a = rs.uniform(-1, 1, (coop.batch_size, m.nu))
    for b in (coop, solo):
      b.set_control(a)
      if between:
        between(b, t)
      launch(b)
    _same(coop, solo, t)
    rows = max(rows, int(coop.get('nefc').max())); solves += int((coop.get('solver_iter') > 0).sum())
  return rows, solves


@pytest.mark.parametrize('B', [1, 2, 3, 5, 8, 9, 23])
@pytest.mark.parametrize('name', nr.BAKED)
def test_fp32_cooperative_stage_is_bit_identical_to_the_one_wave_stage(monkeypatch, name, B):
  m, coop, solo = _pair(monkeypatch, name, B)
  assert coop.info()['launch']['coop_open'] == 1
  rows, solves = _run(m, coop, solo, lambda b: b.step())
  assert rows > 0 and solves > 0 and np.isfinite(coop.get('qpos')).all()
  coop.close(); solo.close()


def test_state_written_through_bound_memory_misses_the_stash_next_to_a_hit(monkeypatch):
  """Three environments of nine get another qpos between launches, written through bound device memory (no notification:
  the stash's own comparison finds them).  Environments 1 and 2 sit in the first wave pair next to 0 and 3, whose stash
  hits: the owner wave runs the full stage for the former while the pair's sides run the latter's."""
  import torch
  m, coop, solo = _pair(monkeypatch, 'cheetah', 9)
  assert coop.info()['launch']['coop_open'] == 1
  q0 = np.ascontiguousarray(nr._init(m, 'cheetah', 9, 1).T)
  bound = {}
  for b in (coop, solo):
    bound[b] = torch.from_numpy(q0).to(torch.float32).cuda()
    torch.cuda.synchronize()
    b.bind('qpos', bound[b].data_ptr())

  def edit(b, t):
    if t % 3 == 1:
      b.sync()
      bound[b][3:, [1, 2, 7]] += 0.02
      torch.cuda.synchronize()
  rows, solves = _run(m, coop, solo, lambda b: b.step(), between=edit)
  assert rows > 0 and solves > 0 and np.isfinite(coop.get('qpos')).all()
  coop.close(); solo.close()


def test_set_qpos_between_launches(monkeypatch):
  m, coop, solo = _pair(monkeypatch, 'cheetah', 9)

  def edit(b, t):
    if t % 4 == 2:
      q = b.get('qpos')
      q[[0, 4, 5], 3:] += 0.03
      b.set('qpos', q)
  _run(m, coop, solo, lambda b: b.step(), between=edit)
  coop.close(); solo.close()


def test_env_mode_mixed_inside_a_pair(monkeypatch):
  m, coop, solo = _pair(monkeypatch, 'cheetah', 9)
  modes = [np.array([[0], [1], [2], [0], [2], [2], [1], [0], [0]], np.int32),      # (wave 2: both environments untouched)
           np.zeros((9, 1), np.int32),
           np.array([[2], [2], [2], [2], [0], [1], [0], [0], [2]], np.int32)]      # (the first pair: nobody steps)

  def edit(b, t):
    b.set('env_mode', modes[t % 3])
  _run(m, coop, solo, lambda b: b.step(), between=edit)
  coop.close(); solo.close()


def test_multi_step_launch_and_forward(monkeypatch):
  m, coop, solo = _pair(monkeypatch, 'cheetah', 9)
  _run(m, coop, solo, lambda b: b.step(4), steps=12)
  _run(m, coop, solo, lambda b: b.forward(), steps=2)
  _run(m, coop, solo, lambda b: b.step(), steps=6)
  coop.close(); solo.close()


def test_bad_qacc_with_auto_reset_retries_on_the_owner_wave(monkeypatch):
  m, coop, solo = _pair(monkeypatch, 'cheetah', 9)
  push = np.zeros((9, m.nv)); push[2, 4] = 1e14      # qacc past mjMAXVAL: mj_checkAcc resets the environment and retries the pass

  def edit(b, t):
    if t in (5, 6):
      b.set('qfrc_applied', push if t == 5 else np.zeros_like(push))
  seen = []

  def launch(b):
    b.step()
    seen.append(b.get('warning'))
  _run(m, coop, solo, launch, between=edit, steps=14)
  w = np.max(seen, axis=0)
  assert w[2, BADQACC] >= 1 and w[[0, 1, 3, 4, 5, 6, 7, 8]][:, [BADQPOS, BADQVEL, BADQACC]].sum() == 0, w
  assert np.isfinite(coop.get('qpos')).all()
  coop.close(); solo.close()


def test_one_wave_workgroups_do_not_cooperate(monkeypatch):
  m, coop, solo = _pair(monkeypatch, 'cheetah', 9, waves=0)
  assert coop.info()['waves_per_block'] == 1 and coop.info()['launch']['coop_open'] == 0
  _run(m, coop, solo, lambda b: b.step(), steps=10)
  coop.close(); solo.close()


def test_fp64_cooperative_stage_is_bit_identical_to_the_one_wave_stage(monkeypatch):
  m, coop, solo = _pair(monkeypatch, 'cheetah', 9, precision=64)
  assert coop.info()['launch']['coop_open'] == 1
  rows, solves = _run(m, coop, solo, lambda b: b.step())
  assert rows > 0 and solves > 0
  coop.close(); solo.close()

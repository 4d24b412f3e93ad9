"""The launch's entry and exit as they move data now -- model tables in one batch of 16-byte loads, the argument structs
carried to LDS by all threads, the kinematic stash as 16-byte pieces of a record with an aligned stride, the state's
exit stores behind one group of LDS reads, the time stored first (step_kernel.hip.h, step_core.h: kWideIO) -- against
the entry and exit they replace: the same sources built with -DDMC_NO_WIDE_IO as an on-demand plugin
(dm_control_amd/specialise.py).

Only data moves differently; no arithmetic instruction of any stage changes.  So every case asks for equality to the
bit of the state (qpos, qvel, qacc_warmstart, act, time), the sensors, the warnings and every output array the launch's
mask stores, after every launch.  The cases are the paths the entry and the exit can take: both precisions, a ragged
last wave, records of odd environments (only 8-byte aligned under the packed stride), a stash that is stale (state
edited, epoch bumped) or absent, the generic kernel (run-time table counts), a model whose tables take several trips
and whose stash is loaded in place, its queued and sliced launch, mj_step1 / mj_step2 on the full stash, launches of
several steps and mj_forward.  B <= 64 and at most 20 launches, but for the queued launch: a queue only exists for a
batch larger than what is resident at once, so that case runs the smallest such batch for two launches."""
import numpy as np
import pytest

import test_gpu_newton_regs as nr
from dm_control_amd.suite import common

pytestmark = pytest.mark.gpu

REF_FLAGS = '-DDMC_NO_WIDE_IO'
STATE = ('qpos', 'qvel', 'qacc_warmstart', 'act', 'time', 'ctrl')
OUTPUTS = ('sensordata', 'warning', 'xpos', 'xquat', 'xmat', 'xipos', 'geom_xpos', 'geom_xmat', 'site_xpos', 'site_xmat',
           'subtree_com', 'qacc', 'actuator_force', 'qfrc_actuator', 'qfrc_bias', 'qfrc_constraint', 'cvel', 'ncon', 'nefc',
           'solver_iter', 'contact_dist', 'contact_pos', 'contact_frame', 'contact_force', 'contact_geom1', 'contact_geom2')
_QUEUE_ENV = ('DMC_SLICES', 'DMC_NO_QUEUE', 'DMC_NO_LPT', 'DMC_XCDS', 'DMC_NO_KSTASH', 'DMC_WAVES', 'DMC_JLEVEL', 'DMC_STASH')


def _batch(monkeypatch, m, B, precision, flags, caps=None, env=None):
  """flags None: the kernel a user gets (baked for a suite model that has one); a string: the plugin of these sources
  built with it, the baked kernel hidden.  env: library switches read when the batch is created."""
  from dm_control_amd.batch import BatchedPhysics
  for v in _QUEUE_ENV + ('DMC_SPEC_PLUGIN', 'DMC_SPEC_FLAGS', 'DMC_NO_STATIC'):
    monkeypatch.delenv(v, raising=False)
  for k, v in (env or {}).items():
    monkeypatch.setenv(k, v)
  if flags is None:
    b = BatchedPhysics(m, B, precision=precision, **(caps or {}))
  else:
    monkeypatch.setenv('DMC_NO_STATIC', '1')
    monkeypatch.setenv('DMC_SPEC_FLAGS', flags)
    b = BatchedPhysics(m, B, precision=precision, specialise='build', **(caps or {}))
    monkeypatch.delenv('DMC_NO_STATIC')
    monkeypatch.delenv('DMC_SPEC_FLAGS')
    assert b.specialised == 'attached' and b.info()['static_id'] == 1000, b.info()
  for k in (env or {}):
    monkeypatch.delenv(k)
  return b


def _pair(monkeypatch, name, B, precision, env=None, baked=True):
  """(new entry / exit, the one it replaces) of one model; baked: the first is the library's own kernel of the model."""
  m = nr._model(name)
  caps = dict(common.DEFAULT_CAPS.get(name, {}))
  caps.pop('precision', None)
  new = _batch(monkeypatch, m, B, precision, None if baked else '', caps, env)
  if baked:
    assert 0 <= new.info()['static_id'] < 1000, new.info()
  ref = _batch(monkeypatch, m, B, precision, REF_FLAGS, caps, env)
  assert ref.info()['lanes_per_env'] == new.info()['lanes_per_env'] and ref.info()['work_queue'] == new.info()['work_queue']
  q = _init(m, name, B)
  for b in (new, ref):
    b.set('qpos', q)
  return m, new, ref


def _init(m, name, B):
  """Start states: the small models' as tests/test_gpu_newton_regs.py draws them; a model with a free joint stands as its
  qpos0 has it with every limited hinge drawn from the middle third of its range (so that the environments differ)."""
  if m.nq == m.njnt:
    return nr._init(m, name, B, 1)
  rs = np.random.RandomState(1)
  q = np.tile(m.qpos0, (B, 1))
  lim = np.flatnonzero(m.jnt_limited == 1)
  lo, hi = m.jnt_range[lim].T
  mid, half = (lo + hi) / 2, (hi - lo) / 6
  q[:, m.jnt_qposadr[lim]] = rs.uniform(mid - half, mid + half, (B, lim.size))
  return q


# what the acceleration stage writes: an mj_step1 launch stores these rows from LDS slots it never wrote (whatever the
# workgroup that held the CU before left there -- in either build), so they are not compared after one
ACC_STAGE = ('qacc', 'actuator_force', 'qfrc_actuator', 'qfrc_constraint', 'contact_force')


def _same(new, ref, what, skip=()):
  m = new.model
  diff = []
  for f in STATE + OUTPUTS:
    if (f == 'act' and not m.na) or f in skip:
      continue
    x, y = new.get(f), ref.get(f)
    if x.tobytes() != y.tobytes():
      diff.append((f, int((x != y).sum())))
  assert not diff, '%s: fields that differ (elements): %s' % (what, diff)


def _drive(new, ref, launches, seed=2, launch=lambda b: b.step(), first=0):
  rs = np.random.RandomState(seed)
  m = new.model
  for t in range(first, first + launches):
    a = rs.uniform(-1, 1, (new.batch_size, m.nu))
    for b in (new, ref):
      b.set_control(a)
      launch(b)
    _same(new, ref, 'launch %d' % t)
  assert np.isfinite(new.get('qpos')).all()


@pytest.mark.parametrize('precision', [32, 64])
def test_cheetah_every_field_after_every_launch(monkeypatch, precision):
  m, new, ref = _pair(monkeypatch, 'cheetah', 64, precision)
  _drive(new, ref, 20)
  assert float(new.get('time').min()) > 0
  new.close(); ref.close()


@pytest.mark.parametrize('B', [1, 5, 9])
def test_ragged_last_wave(monkeypatch, B):
  m, new, ref = _pair(monkeypatch, 'cheetah', B, 32)
  _drive(new, ref, 6)
  new.close(); ref.close()


@pytest.mark.parametrize('which', ['all', 'odd'])
def test_state_edit_between_launches_makes_the_stash_stale(monkeypatch, which):
  """odd: only the odd environments are edited -- their records sit at an 8-byte phase under the packed stride -- so the
  even ones take their stash back and the odd ones recompute, side by side in one wave."""
  m, new, ref = _pair(monkeypatch, 'cheetah', 64, 32)
  _drive(new, ref, 4)
  rs = np.random.RandomState(5)
  sel = slice(None) if which == 'all' else slice(1, None, 2)
  for f, n in (('qpos', m.nq), ('qvel', m.nv)):
    x = new.get(f)
    x[sel] += rs.uniform(-.05, .05, x[sel].shape)
    for b in (new, ref):
      b.set(f, x)
  _drive(new, ref, 4, seed=3, first=4)
  new.close(); ref.close()


def test_epoch_bump_between_launches(monkeypatch):
  m, new, ref = _pair(monkeypatch, 'walker', 64, 32)
  _drive(new, ref, 3)
  for b in (new, ref):
    b.invalidate()
  _drive(new, ref, 3, seed=3, first=3)
  new.close(); ref.close()


def test_without_the_kinematic_stash(monkeypatch):
  m, new, ref = _pair(monkeypatch, 'cheetah', 64, 32, env={'DMC_NO_KSTASH': '1'})
  _drive(new, ref, 6)
  new.close(); ref.close()


@pytest.mark.parametrize('name', ['hopper', 'cartpole'])
def test_generic_kernel_with_run_time_table_counts(monkeypatch, name):
  """The library's generic kernel (the baked one hidden, no plugin) against the plugin of the old entry and exit: two
  compilations of the stages, so in fp64, where nothing is contracted and both round alike.  The hopper's kinematic range
  starts on a 16-byte boundary of its scratch, the cartpole's eight bytes behind one (a partial first piece)."""
  from dm_control_amd.batch import BatchedPhysics
  m = nr._model(name)
  for v in _QUEUE_ENV + ('DMC_SPEC_PLUGIN', 'DMC_SPEC_FLAGS'):
    monkeypatch.delenv(v, raising=False)
  monkeypatch.setenv('DMC_NO_STATIC', '1')
  new = BatchedPhysics(m, 64, precision=64, specialise='off')
  monkeypatch.delenv('DMC_NO_STATIC')
  assert new.info()['static_id'] < 0, new.info()
  ref = _batch(monkeypatch, m, 64, 64, REF_FLAGS)
  q = nr._init(m, name, 64, 1)
  for b in (new, ref):
    b.set('qpos', q)
  _drive(new, ref, 10)
  new.close(); ref.close()


def test_large_model_tables_in_several_trips_and_state_in_place(monkeypatch):
  """humanoid_CMU: n_mr_lds < n_mr (the cold tables stay in global memory; the hot ones take several trips of the
  workgroup), nq = 63 of the group's 64 lanes, and a kinematic range no prefetch register holds (a generic-size range:
  the stash is loaded in place).  (No suite model has more coordinates than lanes: the state's in-place loads run under
  the full stash, test_step1_and_step2_on_the_full_stash.)"""
  m, new, ref = _pair(monkeypatch, 'humanoid_CMU', 8, 32, baked=False)
  _drive(new, ref, 2)
  new.close(); ref.close()


def test_large_model_queued_and_sliced(monkeypatch):
  """The smallest batch of humanoid_CMU that runs from the work queues, three physics steps per launch: items claimed
  after a wave's first load in place, and (where the device cuts items into pieces) travel through the hand-off record."""
  import torch
  m = nr._model('humanoid_CMU')
  probe = _batch(monkeypatch, m, 4096, 32, '', dict(nconmax=96))
  info = probe.info()
  probe.close()
  resident = torch.cuda.get_device_properties(0).multi_processor_count * info['envs_per_cu']
  if info['work_queue']:
    resident = max(resident, info['grid'] * info['envs_per_block'])
  B = resident + 3 * info['envs_per_block'] + 1
  m, new, ref = _pair(monkeypatch, 'humanoid_CMU', B, 32, baked=False)
  assert new.info()['work_queue'] == 1, new.info()
  print('measured: queued batch %d, slices %d' % (B, new.info()['slices']))
  _drive(new, ref, 2, launch=lambda b: b.step(3))
  new.close(); ref.close()


def test_step1_and_step2_on_the_full_stash(monkeypatch):
  m, new, ref = _pair(monkeypatch, 'cheetah', 64, 32)
  for b in (new, ref):
    b.set_opt('stash', 1)
    b.forward()
  _same(new, ref, 'forward')
  rs = np.random.RandomState(4)
  for t in range(5):
    a = rs.uniform(-1, 1, (64, m.nu))
    for b in (new, ref):
      b.set_control(a)
      b.step2()
    _same(new, ref, 'mj_step2 %d' % t)
    for b in (new, ref):
      b.step1()
    _same(new, ref, 'mj_step1 %d' % t, skip=ACC_STAGE)
  new.close(); ref.close()


def test_three_step_launches(monkeypatch):
  m, new, ref = _pair(monkeypatch, 'hopper', 64, 32)
  _drive(new, ref, 6, launch=lambda b: b.step(3))
  new.close(); ref.close()


def test_mj_forward(monkeypatch):
  m, new, ref = _pair(monkeypatch, 'walker', 64, 32)
  _drive(new, ref, 2)
  _drive(new, ref, 3, seed=6, launch=lambda b: b.forward(), first=2)
  new.close(); ref.close()


def test_the_stash_is_taken_back(monkeypatch):
  """Equal results do not show that the 16-byte stash path was taken: a stash that never validates recomputes the
  kinematics to the same bits.  What shows it is time.  The wave trace (dmc_batch_wave_trace) stamps every wave when it
  starts its item and after the first integration; in between lie the opening position / velocity stage and the
  acceleration stage.  The batch first settles under zero control in one launch of 300 steps, so that the solver's work
  no longer changes from launch to launch; then eight launches alternate between one behind an epoch bump (every record
  stale: kinematics, COM frame and velocities recomputed) and one without (every record valid: the three passes
  skipped).  The bound is the sign alone -- the median of the valid launches' waves is shorter than that of the stale
  ones', in the new kernel as in the old one -- and the medians are printed."""
  m, new, ref = _pair(monkeypatch, 'cheetah', 64, 32)
  med = {}
  for tag, b in (('new', new), ('old', ref)):
    b.set_control(np.zeros((64, m.nu)))
    b.step(300)
    b.step()
    b.wave_trace(True)
    for t in range(8):
      if t % 2 == 0:
        b.invalidate()
      b.step()
    b.sync()
    tr = b.wave_trace().astype(np.int64)
    span = (tr[:, 6] - tr[:, 1]) & 0x7fffffff      # (slot = launch since enabling, wave): ticks of 10 ns
    med[tag] = (float(np.median(span[0::2])), float(np.median(span[1::2])))
    b.wave_trace(False)
  print('measured: start of the item to the end of the first integration, median ticks of 10 ns over 4 launches x 32 '
        'waves, (stale, valid): %s' % med)
  _same(new, ref, 'after the traced launches')
  for tag, (stale, valid) in med.items():
    assert valid < stale, (tag, med)
  new.close(); ref.close()

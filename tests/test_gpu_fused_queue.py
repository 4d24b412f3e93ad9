"""suite/fused_env.py `inline=True` -- the generated task layer as the epilogue of the step kernel -- in the launch shapes the
other modules leave out: a batch larger than the device holds at once (a resident grid whose waves claim environments from
the device queues) whose environments are handed out in pieces of physics steps (StepIO::slices), the ragged last wave of a
two-environments-per-wave kernel, and a lean task kernel asked for an optional launch feature.

The epilogue reads most of its inputs from the LDS slot of the wave that runs it.  In a sliced launch that wave is the one
that runs an environment's LAST piece, so whatever the environment did in that launch -- `nstep` physics steps, or the
single mj_forward pass of an episode's first step -- must have left its arrays in that wave's slot."""
import numpy as np
import pytest

from dm_control_amd import suite
from test_fused_env import _make, _port_eval

pytestmark = pytest.mark.gpu

_QUEUE_ENV = ('DMC_SLICES', 'DMC_NO_QUEUE', 'DMC_NO_LPT', 'DMC_XCDS')
_queued = {}


def _queued_batch_size(domain, task, precision):
  """The smallest batch of this model that the device at hand runs from its work queues: what is resident at once plus a
  few workgroups.  Returns (B, control timestep)."""
  import torch
  key = (domain, task, precision)
  if key not in _queued:
    host = suite.load(domain, task, task_kwargs=dict(random=0), physics_kwargs=dict(batch_size=4096, precision=precision))
    info = host.physics.batch.info()
    dt = float(host.control_timestep())
    host.physics.free()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    resident = ncu * info['envs_per_cu']
    if info['work_queue']:      # (the launch of a queued batch IS the resident workgroups)
      resident = max(resident, info['grid'] * info['envs_per_block'])
    _queued[key] = (resident + 3 * info['envs_per_block'] + 1, dt)      # (+ 1: the batch is no whole number of workgroups)
  B, dt = _queued[key]
  assert B < 4096, (B, 'the workload batch itself is barely queued on this device')
  return B, dt


def _require_slices(env, info):
  """The launches of `env` are cut into pieces -- or the test is skipped with the reason (a device whose L2 arrangement the
  library judged unsafe for pieces runs whole items, and nothing here forces it to do otherwise)."""
  if info['slices'] <= 1:
    env.close()
    pytest.skip('this device runs whole items (dmc_batch_info slices = %d): no sliced launch to test' % info['slices'])
  assert min(env.n_sub_steps, info['slices']) > 1, (env.n_sub_steps, info)


def _state_log(env):
  t = env._tensors
  return [x.cpu().numpy().copy() for x in (env.obs, env.reward, env.done, env.first, env.discount, env.terminated, env.steps,
                                           env.episode, t['qpos'], t['qvel'])]


_LOG_NAMES = ('obs', 'reward', 'done', 'first', 'discount', 'terminated', 'steps', 'episode', 'qpos', 'qvel')


def test_inline_epilogue_on_a_queued_sliced_launch_equals_the_host_port(monkeypatch):
  """(a) fp64 humanoid stand, inline, on the smallest queued batch: before every step after the first a fifth of the
  environments is restarted, so every launch mixes environments that take mj_forward under the launch override (one pass)
  with environments that step (n_sub_steps physics steps in pieces), and every environment has a first step inside such a
  launch.  Observation and reward of EVERY environment against the host port on the device's state, 1e-9 (the figure of
  tests/test_fused_env.py for this comparison); reward exactly 0, `first`, and the step counters as control.Environment
  counts them.  (Before the override's pass moved to the last piece: B = 1037, 1031 first observations wrong by up to 2.8.)"""
  import torch
  for k in _QUEUE_ENV:
    monkeypatch.delenv(k, raising=False)
  B, _ = _queued_batch_size('humanoid', 'stand', 64)
  env = _make('humanoid', 'stand', B, precision=64, inline=True, pool_rounds=2)
  info = env.host_physics.batch.info()
  assert env.inline and info['static_id'] == 1000 and info['work_queue'] == 1, info
  _require_slices(env, info)
  assert env.step_limit > 6      # (no episode ends by itself: the reference needs no exclusions)
  rs = np.random.RandomState(21)
  e = np.arange(B)
  steps = np.zeros(B, np.int64)
  for k in range(6):
    mask = np.ones(B, bool) if k == 0 else (e % 5 == k % 5)
    if k:
      env.restart(torch.as_tensor(mask, device='cuda'))
    obs, rew, done = env.step(torch.as_tensor(rs.uniform(-1, 1, (B, env.model.nu)), device='cuda'))
    torch.cuda.synchronize()
    steps = np.where(mask, 0, steps + 1)
    first = env.first.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(first, mask, err_msg='first, step %d' % k)
    np.testing.assert_array_equal(env.steps.cpu().numpy(), steps, err_msg='steps, step %d' % k)
    assert not bool(done.any())
    for name, live in env._attr_live.items():      # the port reads the episode's attributes (targets ...) off the physics
      host = getattr(env.host_physics, name)
      setattr(env.host_physics, name, live.cpu().numpy().astype(np.float64).reshape(host.shape))
    want_obs, want_rew = _port_eval(env.host_env, B)
    got_obs, got_rew = obs.cpu().numpy(), rew.cpu().numpy()
    bad = np.flatnonzero(~np.isclose(got_obs, want_obs, rtol=1e-9, atol=1e-9).all(axis=1))
    print('step %d: %d of %d environments differ from the host port (%d of them first); max |obs - port| = %.3e, max |reward - port| = %.3e'
          % (k, bad.size, B, int(mask[bad].sum()), np.abs(got_obs - want_obs).max(), np.abs(got_rew - np.where(mask, 0, want_rew)).max()))
    np.testing.assert_allclose(got_obs, want_obs, rtol=1e-9, atol=1e-9, err_msg='observation, step %d' % k)
    np.testing.assert_allclose(got_rew, np.where(mask, 0, want_rew), rtol=1e-9, atol=1e-9, err_msg='reward, step %d' % k)
    np.testing.assert_array_equal(got_rew[mask], 0.0)
  assert not env.warnings().any()
  env.close()


@pytest.mark.parametrize('domain', ['humanoid', 'humanoid_CMU'])
def test_launch_shape_does_not_change_a_fused_environment(domain, monkeypatch):
  """(b) fp32 `stand`, inline, a three-step time limit (episodes end inside the epilogue and restart there) and one early
  restart of every seventh environment: the default launch (queue + pieces), two pieces, whole items and the static grid run
  the same kernel object and must give the same bits -- outputs, flags, counters and the bound state -- after every step.
  (Before the override's pass moved to the last piece the sliced variants differed even from each other: humanoid B = 2061,
  2055 first observations; humanoid_CMU B = 1037, 1025.)"""
  import torch
  B, dt = _queued_batch_size(domain, 'stand', 32)
  variants = (('default', {}), ('two_pieces', {'DMC_SLICES': '2'}), ('whole_items', {'DMC_SLICES': '1'}), ('static_grid', {'DMC_NO_QUEUE': '1'}))
  logs, pools = {}, {}
  for name, setting in variants:
    for k in _QUEUE_ENV:
      monkeypatch.delenv(k, raising=False)
    for k, v in setting.items():
      monkeypatch.setenv(k, v)
    env = _make(domain, 'stand', B, precision=32, inline=True, pool_rounds=2, task_kwargs=dict(time_limit=3 * dt))
    info = env.host_physics.batch.info()
    assert env.inline and info['static_id'] == 1000, info
    assert info['work_queue'] == (0 if name == 'static_grid' else 1), (name, info)
    assert env.n_sub_steps > 1 and env.step_limit <= 4
    if name == 'default':
      _require_slices(env, info)
    elif name != 'static_grid':
      assert info['slices'] == int(setting['DMC_SLICES']), (name, info)
    pools[name] = [env._pool[f].cpu().numpy() for f in env._state_names] + [env._attr_pool[k].cpu().numpy() for k in sorted(env._attr_pool)]
    rs = np.random.RandomState(17)
    log = []
    for k in range(8):
      if k == 1:
        env.restart(torch.arange(B, device='cuda') % 7 == 0)      # (out of phase with the rest from here on)
      env.step(torch.as_tensor(rs.uniform(-1, 1, (B, env.model.nu)), dtype=torch.float32, device='cuda'))
      torch.cuda.synchronize()
      log.append(_state_log(env))
    logs[name] = log
    env.close()
  for name, _ in variants[1:]:      # same seed, host RNG: the same start states
    assert len(pools[name]) == len(pools['default'])
    for x, y in zip(pools['default'], pools[name]):
      np.testing.assert_array_equal(x, y, err_msg='pool, ' + name)
  first = np.stack([l[3] for l in logs['default']]).astype(bool)
  assert any(f.any() and not f.all() for f in first)      # (a launch with first steps AND stepping environments)
  assert np.stack([l[2] for l in logs['default']]).any()      # (episodes did end)
  for name, _ in variants[1:]:
    for k, (a, b) in enumerate(zip(logs['default'], logs[name])):
      for what, x, y in zip(_LOG_NAMES, a, b):
        if not np.array_equal(x, y):
          rows = np.flatnonzero((x != y).reshape(-1, B).any(axis=0) if what in ('qpos', 'qvel') else (x != y).reshape(B, -1).any(axis=1))
          print('%s vs default, step %d, %s: %d environments differ (%d of them in their first step)' % (name, k, what, rows.size, int(first[k][rows].sum())))
        np.testing.assert_array_equal(x, y, err_msg='%s vs default: %s after step %d' % (name, what, k))


@pytest.mark.parametrize('B', [41, 1])
def test_ragged_last_wave_under_the_epilogue(B):
  """(c) cheetah (two environments per wave) with an odd batch: the last wave's second slot has no environment.  The
  epilogue inside the kernel against the same function as a kernel of its own, over steps that cross episode ends."""
  import torch
  outs = []
  for inline in (True, False):
    env = _make('cheetah', 'run', B, precision=64, inline=inline, task_kwargs=dict(time_limit=5 * 0.01))
    info = env.host_physics.batch.info()
    assert env.inline == inline and env.step_limit <= 6 and (info['static_id'] == 1000) == inline
    assert info['lanes_per_env'] == 32 and B % 2 == 1      # (two environments per wave: an odd batch ends on half a wave)
    rs = np.random.RandomState(9)
    log = []
    for k in range(8):
      obs, rew, done = env.step(torch.as_tensor(rs.uniform(-1, 1, (B, env.model.nu)), device='cuda'))
      torch.cuda.synchronize()
      log.append([x.cpu().numpy().copy() for x in (obs, rew, done, env.first, env.discount, env.terminated, env.steps, env.episode)])
    outs.append(log)
    assert not env.warnings().any()
    env.close()
  assert np.stack([l[2] for l in outs[0]]).any()      # (episodes did end)
  for a, b in zip(*outs):
    for k, (x, y) in enumerate(zip(a, b)):
      if k < 2:
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9)
      else:
        np.testing.assert_array_equal(x, y)


def test_lean_task_kernel_refuses_a_launch_it_cannot_take():
  """(d) The task kernel of a lean model (fp32, nv < 30) is built without the optional launch features.  With a substep probe
  set, the launch cannot go to it -- and the library's own kernel knows nothing of the task.  Either the step raises an
  error that names the conflict, or the epilogue ran: `steps` and `first` are written by nothing else.  (Before the
  refusal: the step returned with `first` = 0 and `steps` = 0 for every environment, and no error.)"""
  import torch
  from dm_control_amd import _native
  B = 40
  env = _make('cheetah', 'run', B, precision=32, inline=True)
  assert env.inline and env.host_physics.batch.info()['static_id'] == 1000
  probe = torch.zeros((env.n_sub_steps, 3, B), dtype=torch.float32, device='cuda')
  env.host_physics.batch.set_step_probe(env.host_physics.batch.model.name2id('torso', 'geom'), probe.data_ptr(), env.n_sub_steps)
  rs = np.random.RandomState(2)
  try:
    for k in range(4):
      try:
        env.step(torch.as_tensor(rs.uniform(-1, 1, (B, env.model.nu)), dtype=torch.float32, device='cuda'))
      except _native.NativeError as ex:
        assert 'task' in str(ex) and 'optional launch features' in str(ex), str(ex)
        return
      torch.cuda.synchronize()
      # (no refusal: then the task layer must have run -- step 0 is every episode's first, step k its k-th after that)
      np.testing.assert_array_equal(env.first.cpu().numpy(), np.full(B, 1 if k == 0 else 0, np.uint8), err_msg='first, step %d: the epilogue did not run' % k)
      np.testing.assert_array_equal(env.steps.cpu().numpy(), np.full(B, k, np.int32), err_msg='steps, step %d: the epilogue did not run' % k)
  finally:
    env.host_physics.batch.set_step_probe(0, None, 0)
    env.close()

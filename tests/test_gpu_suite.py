"""Drop-in surface on the GPU: `suite.load`, the `Physics` facade and the tasks,
checked against the oracle and against the reference's suite-level properties
(dm_control/suite/suite_test.py: spec conformance :149, determinism :170, finite
observations :81, reward range :94)."""
import numpy as np
import pytest

from dm_control_amd import mjcf_compiler as mc

pytestmark = pytest.mark.gpu


def _oracle(model):
  from oracle.oracle import OraclePhysics
  return OraclePhysics(model)


@pytest.mark.parametrize('domain,task', [('cheetah', 'run'), ('cartpole', 'balance'), ('cartpole', 'swingup'),
                                         ('humanoid', 'stand'), ('humanoid', 'run_pure_state'), ('walker', 'walk'),
                                         ('hopper', 'hop'), ('hopper', 'stand'), ('pendulum', 'swingup'),
                                         ('acrobot', 'swingup'), ('acrobot', 'swingup_sparse'),
                                         ('finger', 'spin'), ('finger', 'turn_easy'), ('finger', 'turn_hard'),
                                         ('reacher', 'easy'), ('reacher', 'hard'),
                                         ('point_mass', 'easy'), ('point_mass', 'hard'),
                                         ('ball_in_cup', 'catch'), ('fish', 'upright'), ('fish', 'swim'),
                                         ('manipulator', 'bring_ball'), ('manipulator', 'bring_peg'),
                                         ('manipulator', 'insert_ball'), ('swimmer', 'swimmer6'),
                                         ('swimmer', 'swimmer15'), ('humanoid_CMU', 'stand'), ('humanoid_CMU', 'run'),
                                         ('quadruped', 'walk'), ('quadruped', 'fetch'), ('stacker', 'stack_2'),
                                         ('stacker', 'stack_4'), ('manipulator', 'insert_peg')])
def test_suite_task_properties(domain, task):
  from dm_control_amd import suite
  env = suite.load(domain, task, task_kwargs=dict(random=0))
  aspec = env.action_spec()
  rs = np.random.RandomState(1)
  ts = env.reset()
  assert ts.first()
  ospec = env.observation_spec()
  n = 0
  while not ts.last() and n < 60:
    action = rs.uniform(aspec.minimum, aspec.maximum, aspec.shape)
    ts = env.step(action)
    n += 1
    assert set(ts.observation) == set(ospec)
    for k, v in ts.observation.items():
      v = np.asarray(v)
      assert v.shape == ospec[k].shape and np.all(np.isfinite(v)), k
    assert 0.0 <= ts.reward <= 1.0
  env.physics.free()


@pytest.mark.parametrize('domain,task', [('cheetah', 'run'), ('cartpole', 'swingup'), ('humanoid', 'walk'),
                                         ('walker', 'run'), ('hopper', 'hop'), ('acrobot', 'swingup'),
                                         ('finger', 'turn_hard'), ('reacher', 'hard'), ('point_mass', 'hard'),
                                         ('fish', 'swim'), ('swimmer', 'swimmer6'), ('lqr', 'lqr_6_2'),
                                         ('ball_in_cup', 'catch'), ('manipulator', 'bring_ball'),
                                         ('humanoid_CMU', 'walk'), ('quadruped', 'run'), ('stacker', 'stack_2')])
def test_same_seed_same_trajectory(domain, task):
  from dm_control_amd import suite

  def rollout():
    env = suite.load(domain, task, task_kwargs=dict(random=42))
    aspec = env.action_spec()
    rs = np.random.RandomState(7)
    ts = env.reset()
    out = [np.concatenate([np.ravel(v) for v in ts.observation.values()])]
    for _ in range(30):
      ts = env.step(rs.uniform(aspec.minimum, aspec.maximum, aspec.shape))
      out.append(np.concatenate([np.ravel(v) for v in ts.observation.values()] + [[ts.reward]]))
    env.physics.free()
    return out
  a, b = rollout(), rollout()
  for x, y in zip(a, b):
    np.testing.assert_array_equal(x, y)


def test_cheetah_env_matches_oracle_driven_reference_loop():
  """BASELINE config 2 through the full drop-in stack (suite.load -> Environment
  -> Physics facade -> C-ABI -> HIP kernel, fp64) against the same episode played
  on the CPU oracle."""
  from dm_control_amd import suite
  env = suite.load('cheetah', 'run', task_kwargs=dict(random=3))
  ts = env.reset()
  m = env.physics.model
  o = _oracle(m)
  r = np.random.RandomState(3)
  lim = m.jnt_limited == 1
  lo, hi = m.jnt_range[lim].T
  o.reset()
  o.qpos[lim] = r.uniform(lo, hi)
  o.after_reset()
  o.step(200)
  o.time = 0
  np.testing.assert_allclose(ts.observation['position'], o.qpos[1:], atol=1e-10)
  rs = np.random.RandomState(11)
  for t in range(200):
    a = rs.uniform(-1, 1, m.nu)
    ts = env.step(a)
    o.set_control(a)
    o.step()
    np.testing.assert_allclose(ts.observation['position'], o.qpos[1:], atol=1e-9, err_msg=str(t))
    np.testing.assert_allclose(ts.observation['velocity'], o.qvel, atol=1e-7)
    speed = o.sensordata[0]
    want = float(np.clip(speed / 10.0, 0, 1))
    assert abs(ts.reward - want) < 1e-9
  assert abs(env.physics.time() - 2.0) < 1e-9
  env.physics.free()


def test_cartpole_balance_config0_zero_actions_1000_steps():
  """BASELINE config 0: suite cartpole balance, zero actions, 1000 steps (RK4)."""
  from dm_control_amd import suite
  env = suite.load('cartpole', 'balance', task_kwargs=dict(random=0))
  ts = env.reset()
  m = env.physics.model
  assert m.opt.integrator == 1
  o = _oracle(m)
  r = np.random.RandomState(0)
  o.reset()
  o.qpos[0] = r.uniform(-.1, .1)
  o.qpos[1:] = r.uniform(-.034, .034, m.nv - 1)
  o.qvel[:] = 0.01 * r.randn(m.nv)
  o.after_reset()
  n = 0
  while not ts.last():
    ts = env.step(np.zeros(1))
    o.set_control(np.zeros(1))
    o.step()
    n += 1
  assert n == 1000
  np.testing.assert_allclose(env.physics.data.qpos, o.qpos, atol=1e-9)
  np.testing.assert_allclose(env.physics.data.qvel, o.qvel, atol=1e-8)
  env.physics.free()


def test_humanoid_forward_all_sensors_match_oracle():
  """Config 3 model: every sensor (incl. accelerometer / force / torque / touch,
  i.e. rnePostConstraint + contact wrench decoding) on random contact-rich states."""
  from dm_control_amd import suite
  from dm_control_amd.batch import BatchedPhysics
  m = mc.compile_xml(suite.humanoid.get_model_and_assets()[0])
  NE = 24
  rs = np.random.RandomState(0)
  q = np.tile(m.qpos0, (NE, 1))
  q[:, 2] = rs.uniform(0.05, 1.3, NE)
  quat = rs.randn(NE, 4)
  q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
  q[:, 7:] += rs.uniform(-0.4, 0.4, (NE, m.nq - 7))
  v = rs.uniform(-2, 2, (NE, m.nv))
  c = rs.uniform(-1, 1, (NE, m.nu))
  b = BatchedPhysics(m, NE, precision=64, nconmax=48)
  b.set('qpos', q); b.set('qvel', v); b.set('ctrl', c)
  b.forward()
  sens = b.get('sensordata')
  ncon = b.get('ncon')[:, 0]
  qacc = b.get('qacc')
  assert not b.get('warning').any()
  touched = 0
  for e in range(NE):
    o = _oracle(m)
    o.qpos[:], o.qvel[:], o.ctrl[:] = q[e], v[e], c[e]
    o.forward()
    assert o.ncon == ncon[e]
    np.testing.assert_allclose(qacc[e], o.qacc, rtol=1e-8, atol=1e-6)
    scale = max(1.0, np.abs(o.sensordata).max())
    np.testing.assert_allclose(sens[e], o.sensordata, atol=1e-8 * scale, err_msg='env %d' % e)
    touched += int((o.sensordata[48:] > 0).sum())
  assert touched > 0, 'test states never exercised a touch sensor'
  b.close()


@pytest.mark.parametrize('precision,tol', [(64, 1e-10), (32, 2e-4)])   # measured 2.8e-13 / 3.8e-5
def test_humanoid_short_rollout(precision, tol):
  """Humanoid is strongly chaotic (error grows ~10x per 0.5 s), so open-loop parity
  is asserted over 100 physics steps (20 env-steps of 5 substeps)."""
  from dm_control_amd import suite
  from dm_control_amd.batch import BatchedPhysics
  from oracle import oracle
  m = mc.compile_xml(suite.humanoid.get_model_and_assets()[0])
  NE = 8
  rs = np.random.RandomState(2)
  q = np.tile(m.qpos0, (NE, 1))
  q[:, 2] = rs.uniform(1.0, 1.4, NE)
  q[:, 7:] += rs.uniform(-0.2, 0.2, (NE, m.nq - 7))
  b = BatchedPhysics(m, NE, precision=precision, nconmax=48)
  b.set('qpos', q)
  refs = []
  for e in range(NE):
    o = _oracle(m)
    o.qpos[:] = q[e]
    o.forward()
    refs.append(o)
  for t in range(20):
    a = rs.uniform(-1, 1, (NE, m.nu))
    b.set_control(a)
    b.step(5)
    oracle.rollout_legacy(refs, a[None], nsub=5)
  qg = b.get('qpos')
  qo = np.stack([o.qpos for o in refs])
  err = np.abs(qg - qo).max()
  print('measured: humanoid_short_rollout precision=%d max|dqpos|=%.3g' % (precision, err))
  assert err < tol, err
  assert not b.get('warning').any()
  b.close()


def test_physics_facade_semantics():
  from dm_control_amd import physics as pl
  from dm_control_amd.envs import control
  from dm_control_amd import suite
  xml = suite.cheetah.get_model_and_assets()[0]
  p = pl.Physics.from_xml_string(xml)
  assert p.data.qpos.shape == (9,) and p.data.xpos.shape == (8, 3)
  assert p.named.data.qpos['rootz'].shape == (1,)
  z0 = p.named.data.xpos['torso', 'z']
  with p.reset_context():
    p.named.data.qpos['rootz'] = -0.1
  assert abs(p.named.data.xpos['torso', 'z'] - (z0 - 0.1)) < 1e-12
  # state get/set + copy continue identically (engine_test.py:549-572)
  p.set_control(np.full(6, 0.3))
  p.step(5)
  q = p.copy()
  for _ in range(5):
    p.step(); q.step()
  np.testing.assert_array_equal(p.get_state(), q.get_state())
  assert p.time() == q.time()
  s = p.get_state()
  p.reset()
  assert p.time() == 0 and np.array_equal(p.data.qpos, p.model.qpos0)
  p.set_state(s)
  p.forward()
  np.testing.assert_array_equal(p.get_state(), s)
  # invalid state -> PhysicsError naming the warning; suppressed -> no raise
  p.data.qpos[0] = np.inf
  with pytest.raises(control.PhysicsError, match='mjWARN_BADQPOS'):
    p.step()
  p.data.qpos[0] = np.nan
  with p.suppress_physics_errors():
    p.step()
  # action spec (engine_test.py:606-625)
  spec = pl.action_spec(p)
  np.testing.assert_array_equal(spec.minimum, -np.ones(6))
  p.free(); q.free()


def test_timestep_edit_moves_time_by_the_new_timestep():
  """model.opt.timestep edited at run time (engine.py:326-333 reads it back as physics.timestep()): the dynamics AND
  the time accumulator of the device use the new value (the accumulator keeps its own fp64 copy of dt)."""
  from dm_control_amd import physics as pl
  from dm_control_amd import suite
  xml = suite.cheetah.get_model_and_assets()[0]
  for precision in (64, 32):
    p = pl.Physics.from_xml_string(xml, precision=precision)
    dt0 = p.timestep()
    p.step(3)
    t0 = p.data.time
    assert abs(t0 - 3 * dt0) < 1e-12
    p.model.opt.timestep = 0.5 * dt0
    p.step(4)
    assert abs(p.data.time - t0 - 2 * dt0) < 1e-12, (p.data.time, t0, dt0)
    assert p.timestep() == 0.5 * dt0
    p.free()


def test_batched_facade_matches_single():
  from dm_control_amd import physics as pl
  from dm_control_amd import suite
  xml = suite.cheetah.get_model_and_assets()[0]
  single = pl.Physics.from_xml_string(xml)
  batch = pl.Physics.from_xml_string(xml, batch_size=3)
  assert batch.data.qpos.shape == (3, 9) and batch.data.xmat.shape == (3, 8, 9)
  a = np.array([0.2, -0.4, 0.1, 0.9, -1.0, 0.5])
  single.set_control(a)
  batch.set_control(np.tile(a, (3, 1)))
  single.step(7); batch.step(7)
  for e in range(3):
    np.testing.assert_array_equal(batch.data.qpos[e], single.data.qpos)
  np.testing.assert_array_equal(batch.named.data.xpos['torso', 'z'], np.full(3, single.named.data.xpos['torso', 'z']))
  single.free(); batch.free()


def test_torch_batched_env_matches_host_env_semantics():
  """Device-resident cheetah env: observations/rewards equal the host task's
  formulas on the same device state; episodes end at the time limit and reset."""
  import torch
  from dm_control_amd.suite import torch_env, rewards
  env = torch_env.TorchBatchedEnv(64, precision=32, time_limit=0.05, seed=1)
  obs = env.reset()
  assert obs.shape == (64, 17) and torch.isfinite(obs).all()
  g = torch.Generator(device='cuda').manual_seed(0)
  for t in range(5):
    a = torch.rand((64, 6), device='cuda', generator=g) * 2 - 1
    obs, rew, done = env.step(a)
    q = env.physics.get('qpos'); v = env.physics.get('qvel'); s = env.physics.get('sensordata')
    if t < 4:
      np.testing.assert_allclose(obs.cpu().numpy(), np.concatenate([q[:, 1:], v], axis=1), rtol=1e-6, atol=1e-6)
      want = rewards.tolerance(s[:, 0], bounds=(10, float('inf')), margin=10, value_at_margin=0, sigmoid='linear')
      np.testing.assert_allclose(rew.cpu().numpy(), want, atol=1e-6)
      assert not bool(done.any())
  assert bool(done.all())              # 0.05 s / 0.01 s = 5 steps
  assert int(env.steps.max()) == 0     # auto-reset
  assert float(env.time.max()) == 0.0
  env.close()


def test_torch_env_captured_graph_equals_eager_across_a_restart():
  """`capture=True`: the steps in which no environment can reach the time limit are replays of one HIP graph, the others
  (the restart among them) run eagerly.  Same seed, same actions: observation, reward and done of every step equal the
  eager environment's bit for bit (the same kernels in the same order on the same start states: the draws are keyed by
  seed and per-environment draw count) -- over a 5-step time limit crossed twice."""
  import torch
  from dm_control_amd.suite import torch_env
  B = 64
  outs = []
  for capture in (False, True):
    env = torch_env.make('cheetah', 'run', B, precision=32, seed=1, time_limit=0.05, capture=capture)
    assert env.step_limit == 5
    g = torch.Generator(device='cuda').manual_seed(0)
    log = []
    for _ in range(13):
      obs, rew, done = env.step(torch.rand((B, env.model.nu), device='cuda', generator=g) * 2 - 1)
      log.append((obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
    outs.append(log)
    env.close()
  for a, b in zip(*outs):
    for x, y in zip(a, b):
      np.testing.assert_array_equal(x, y)
  done = np.stack([l[2] for l in outs[1]])      # (step, env)
  assert done[[4, 9]].all() and not done[[0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12]].any()
  assert all(np.isfinite(l[0]).all() for l in outs[1])


@pytest.mark.parametrize('name,nsub', [('walker', 10), ('hopper', 4), ('pendulum', 1), ('acrobot', 1),
                                       ('finger', 2), ('reacher', 1), ('point_mass', 1), ('fish', 10), ('ball_in_cup', 10),
                                       ('swimmer6', 15), ('quadruped', 4), ('stacker', 10), ('manipulator', 10)])
def test_more_domains_rollout_parity(name, nsub):
  """Domains sharing the cheetah feature set: 60 env-steps from randomised starts
  against the oracle (fp64 kernel), incl. hopper's touch sensors, acrobot's RK4,
  finger's elliptic cones / dof friction loss / framepos + ellipsoid-site touch sensors, quadruped's filtered
  servos + tendon equalities + ellipsoid torso, and the box contacts of stacker and of the full manipulator model."""
  from dm_control_amd.batch import BatchedPhysics
  from dm_control_amd.suite import common
  from oracle import oracle
  if name.startswith('swimmer'):
    from dm_control_amd.suite import swimmer
    m = mc.compile_xml(swimmer._make_model(int(name[7:])))
  else:
    m = mc.compile_xml(common.read_model(name + '.xml'))
  NE = 8
  rs = np.random.RandomState(5)
  q = np.tile(m.qpos0, (NE, 1))
  for j in range(m.njnt):
    a = m.jnt_qposadr[j]
    if m.jnt_type[j] == 3:
      lo, hi = m.jnt_range[j] if m.jnt_limited[j] else (-np.pi, np.pi)
      q[:, a] = rs.uniform(lo, hi, NE)
  b = BatchedPhysics(m, NE, precision=64, **dict(dict(manipulator=dict(nconmax=40)).get(name, common.DEFAULT_CAPS.get(name, {}))))
  b.set('qpos', q)
  refs = []
  for e in range(NE):
    o = _oracle(m)
    o.qpos[:] = q[e]
    o.forward()
    refs.append(o)
  worst = 0.0
  for t in range(60):
    a = rs.uniform(-1, 1, (NE, m.nu))
    b.set_control(a)
    b.step(nsub)
    oracle.rollout_legacy(refs, a[None], nsub=nsub)
    qo = np.stack([o.qpos for o in refs])
    worst = max(worst, float(np.abs(b.get('qpos') - qo).max()))
  assert worst < 1e-7, worst
  so = np.stack([o.sensordata for o in refs])
  if m.nsensordata:
    np.testing.assert_allclose(b.get('sensordata'), so, atol=1e-6 * max(1.0, np.abs(so).max()))
  assert not b.get('warning').any()
  b.close()


def test_model_constants_rewritten_between_episodes():
  """Tasks rewrite model arrays through physics.named.model (suite/finger.py:139
  dof_damping); the change must reach the device tables before the next launch."""
  from dm_control_amd.suite import finger
  phys = finger.Physics.from_xml_string(*finger.get_model_and_assets())
  o = _oracle(phys.model)

  def spin_down(p_step, get_v):
    for _ in range(20):
      p_step()
    return get_v()
  phys.data.qvel[2] = 5.0
  o.qvel[2] = 5.0
  o.forward()
  v_gpu = spin_down(phys.step, lambda: float(phys.data.qvel[2]))
  v_ora = spin_down(o.step, lambda: float(o.qvel[2]))
  np.testing.assert_allclose(v_gpu, v_ora, rtol=1e-9)
  phys.named.model.dof_damping['hinge'] = .03
  o.model.field('dof_damping')[2] = .03
  phys.reset(); o.reset(); o.after_reset()
  phys.data.qvel[2] = 5.0
  o.qvel[2] = 5.0
  phys.forward(); o.forward()
  v_gpu2 = spin_down(phys.step, lambda: float(phys.data.qvel[2]))
  v_ora2 = spin_down(o.step, lambda: float(o.qvel[2]))
  np.testing.assert_allclose(v_gpu2, v_ora2, rtol=1e-9)
  assert v_gpu2 > v_gpu          # less damping: spins down more slowly
  with pytest.raises(Exception):
    phys.batch.set_model_real('body_mass', phys.model.body_mass)
  phys.free()


def test_cylinder_pairs_are_guarded_not_silently_ignored():
  """A cylinder has a narrow phase against a plane, a sphere and a capsule (tests/test_cylinder_contacts.py); two
  cylinders coming within range of each other (tested as their enclosing capsules) raise the dmcWARN_COLLISION counter
  instead of a contact; a box or an ellipsoid against a cylinder is refused when the batch is created."""
  from dm_control_amd.batch import BatchedPhysics
  m = mc.compile_xml("""
  <mujoco><worldbody>
    <geom name='post' type='cylinder' size='.1 .05'/>
    <body name='can' pos='0 0 .6'><freejoint/><geom type='cylinder' size='.1 .1'/></body>
  </worldbody></mujoco>""")
  b = BatchedPhysics(m, 2, precision=64)
  o = _oracle(m)
  o.forward()
  b.step(100); [o.step() for _ in range(100)]
  assert not b.get('warning').any() and not o.warning.any()       # still falling: out of range
  b.step(100); [o.step() for _ in range(100)]
  w = b.get('warning')
  assert (w[:, mc.C['DMC_WARN_COLLISION']] > 0).all() and o.warning[mc.C['DMC_WARN_COLLISION']] > 0
  assert (b.get('ncon') == 0).all() and o.ncon == 0
  np.testing.assert_allclose(b.get('qpos')[0], o.qpos, atol=1e-9)
  b.close()


def test_lqr_domain_linear_dynamics_and_reward():
  """suite lqr: generated mass-spring chain; reward = 1 - (0.5 |q|^2 + 0.5 c |u|^2) (lqr.py:252-258);
  the unforced chain conserves the discrete-time quadratic invariant of semi-implicit Euler closely."""
  from dm_control_amd import suite
  env = suite.load('lqr', 'lqr_6_2', task_kwargs=dict(random=3))
  ts = env.reset()
  q0 = np.asarray(ts.observation['position'])
  np.testing.assert_allclose(np.linalg.norm(q0), np.sqrt(2), rtol=1e-12)
  u = np.array([0.3, -0.2])
  ts = env.step(u)
  q = np.asarray(ts.observation['position'])
  np.testing.assert_allclose(ts.reward, 1 - (0.5 * q @ q + 0.5 * 0.1 * u @ u), rtol=1e-12)
  o = _oracle(env.physics.model)
  o.qpos[:] = q0
  o.forward()
  o.ctrl[:] = u
  o.step()
  np.testing.assert_allclose(q, o.qpos, atol=1e-12)
  env.physics.free()


@pytest.mark.parametrize('domain,task,move_speed', [('humanoid', 'stand', 0), ('humanoid', 'run', 10),
                                                   ('humanoid_CMU', 'stand', 0), ('humanoid_CMU', 'walk', 1)])
def test_torch_humanoid_env_matches_host_task_formulas(domain, task, move_speed):
  """Device-resident humanoid: start states are collision-free, observations
  and rewards equal Humanoid.get_observation / get_reward evaluated on the same device state."""
  import torch
  from dm_control_amd.suite import torch_env, rewards
  B = 48
  cmu = domain == 'humanoid_CMU'
  env = torch_env.make(domain, task, B, precision=32, time_limit=0.08 if cmu else 0.1, seed=2)
  m = env.model
  assert env.n_sub_steps == (10 if cmu else 5) and env.step_limit == 4
  torso, sides, upright_idx = ('thorax', ('l', 'r'), (2, 1)) if cmu else ('torso', ('left_', 'right_'), (2, 2))
  obs = env.reset()
  assert obs.shape == (B, 137 if cmu else 67) and torch.isfinite(obs).all()
  assert int(env.ncon.max()) == 0                       # rejection-sampled: no initial contacts
  g = torch.Generator(device='cuda').manual_seed(0)
  bid = lambda n: m.name2id(n, 'body')
  for t in range(4):
    a = torch.rand((B, m.nu), device='cuda', generator=g) * 2 - 1
    obs, rew, done = env.step(a)
    if t == 3:
      break
    q, v, s = env.physics.get('qpos'), env.physics.get('qvel'), env.physics.get('sensordata')
    xpos = env.physics.get('xpos').reshape(B, -1, 3)
    xmat = env.physics.get('xmat').reshape(B, -1, 3, 3)
    R, tpos = xmat[:, bid(torso)], xpos[:, bid(torso)]
    ext = np.concatenate([np.einsum('bi,bij->bj', xpos[:, bid(sd + lb)] - tpos, R)
                          for sd in sides for lb in ('hand', 'foot')], axis=1)
    adr = m.sensor_adr[m.name2id(torso + '_subtreelinvel', 'sensor')]
    com_vel = s[:, adr:adr + 3]
    head = xpos[:, bid('head'), 2]
    want_obs = np.concatenate([q[:, 7:], head[:, None], ext, R[:, 2, :], com_vel, v], axis=1)
    np.testing.assert_allclose(obs.cpu().numpy(), want_obs, rtol=1e-5, atol=1e-5)
    standing = rewards.tolerance(head, bounds=(1.4, float('inf')), margin=1.4 / 4)
    upright = rewards.tolerance(R[:, upright_idx[0], upright_idx[1]], bounds=(0.9, float('inf')), sigmoid='linear', margin=1.9, value_at_margin=0)
    sc = (4 + rewards.tolerance(a.cpu().numpy(), margin=1, value_at_margin=0, sigmoid='quadratic').mean(axis=1)) / 5
    if move_speed == 0:
      want = sc * standing * upright * rewards.tolerance(com_vel[:, :2], margin=2).mean(axis=1)
    else:
      move = rewards.tolerance(np.linalg.norm(com_vel[:, :2], axis=1), bounds=(move_speed, float('inf')),
                               margin=move_speed, value_at_margin=0, sigmoid='linear')
      want = sc * standing * upright * (5 * move + 1) / 6
    np.testing.assert_allclose(rew.cpu().numpy(), want, rtol=1e-4, atol=1e-5)
    assert not bool(done.any())
  assert bool(done.all()) and int(env.steps.max()) == 0       # time limit reached: auto-reset on device
  assert int(env.ncon.max()) == 0
  env.close()


@pytest.mark.parametrize('qpos,linvel,angvel,local', [
    ([0., 0.], [1.5, 0, 0], [0, 1, 0], False),
    ([0., np.pi], [0.5, 0, 0], [0, 1, 0], False),
    ([0., np.pi], [-0.5, 0, 0], [0, 1, 0], True)])
def test_facade_object_velocity(qpos, linvel, angvel, local):
  # wrapper/core_test.py:340-391 through physics.data.object_velocity, for the geom the reference
  # queries and the site at the same pose
  from dm_control_amd import physics as physics_lib
  phys = physics_lib.Physics.from_xml_string("""
  <mujoco><option><flag contact='disable'/></option><worldbody><body name='cart'>
    <joint type='slide' axis='1 0 0'/>
    <geom name='cart' type='box' size='0.2 0.2 0.2'/>
    <body name='pole'><joint name='hinge' type='hinge' axis='0 1 0'/>
      <geom name='mass' pos='0 0 .5' size='0.04'/>
      <site name='mass' pos='0 0 .5'/></body></body></worldbody></mujoco>""")
  phys.data.qpos[:] = qpos
  phys.data.qvel[:] = [1., 1.]
  phys.forward()
  for kind in ('geom', 'site'):
    v = phys.data.object_velocity('mass', kind, local_frame=local)
    assert v.shape == (2, 3)
    np.testing.assert_allclose(v[0], linvel, atol=1e-9)
    np.testing.assert_allclose(v[1], angvel, atol=1e-9)
  with pytest.raises(ValueError):
    phys.data.object_velocity('mass', 'joint')
  phys.free()


def test_facade_contact_force_equals_weight():
  # wrapper/core_test.py:393-416 through physics.data.contact_force; ids out of range raise
  from dm_control_amd import physics as physics_lib
  phys = physics_lib.Physics.from_xml_string("""
  <mujoco><worldbody>
    <geom name='floor' type='plane' size='1 1 1'/>
    <body name='box' pos='0 0 .1'><freejoint/>
      <geom name='box' type='box' size='.1 .1 .1'/></body>
  </worldbody></mujoco>""")
  phys.legacy_step = False
  for _ in range(50):
    phys.step(10)
  assert int(phys.data.ncon) == 4
  q_before = np.array(phys.data.qpos, copy=True)
  normal = sum(phys.data.contact_force(i)[0, 0] for i in range(4))
  np.testing.assert_allclose(normal, 9.81 * phys.model.body_mass[1], rtol=0, atol=1e-7)
  np.testing.assert_array_equal(q_before, phys.data.qpos)     # a query does not advance the state
  for bad in (-1, 4):
    with pytest.raises(ValueError):
      phys.data.contact_force(bad)
  phys.free()


def test_pickle_and_deepcopy_continue_identically():
  # engine_test.py:549-572: copy / deepcopy / pickle, then ten more steps give identical states
  import copy, pickle
  from dm_control_amd.suite import cheetah
  phys = cheetah.Physics.from_xml_string(*cheetah.get_model_and_assets())
  rs = np.random.RandomState(0)
  for _ in range(20):
    phys.set_control(rs.uniform(-1, 1, 6))
    phys.step()
  clones = [copy.copy(phys), copy.deepcopy(phys), pickle.loads(pickle.dumps(phys))]
  assert all(type(c) is type(phys) for c in clones)
  for _ in range(10):
    a = rs.uniform(-1, 1, 6)
    for p in [phys] + clones:
      p.set_control(a)
      p.step()
  for c in clones:
    np.testing.assert_array_equal(c.data.qpos, phys.data.qpos)
    np.testing.assert_array_equal(c.data.xpos, phys.data.xpos)
    assert c.data.time == phys.data.time
    c.free()
  phys.free()


def test_manipulator_batched_targets_and_receptacle():
  """Batched manipulator: per-environment ghost targets live in the task, the colliding receptacle
  pose is one model constant per episode pushed through dmc_batch_set_model_real."""
  from dm_control_amd import suite
  env = suite.load('manipulator', 'insert_ball', task_kwargs=dict(random=1), physics_kwargs=dict(batch_size=3))
  ts = env.reset()
  tp = np.asarray(ts.observation['target_pos'])
  assert tp.shape == (3, 4)
  np.testing.assert_allclose(tp[0], tp[1])             # insert: the shared receptacle / target pose
  cup = env.physics.model.name2id('cup', 'body')
  np.testing.assert_allclose(np.asarray(env.physics.data.xpos)[:, cup, [0, 2]], tp[:, :2], atol=1e-12)
  assert (np.atleast_1d(env.physics.data.ncon) == 0).all()
  for _ in range(5):
    ts = env.step(np.zeros((3, 5)))
  assert np.asarray(ts.reward).shape == (3,)
  env.physics.free()
  env = suite.load('manipulator', 'bring_ball', task_kwargs=dict(random=1), physics_kwargs=dict(batch_size=3))
  tp = np.asarray(env.reset().observation['target_pos'])
  assert not np.allclose(tp[0], tp[1])                 # bring: one target per environment
  env.physics.free()


@pytest.mark.parametrize('name,nsub', [('finger', 2), ('fish', 10), ('swimmer6', 15), ('ball_in_cup', 10),
                                       ('manipulator', 10), ('point_mass', 1), ('walker', 10), ('hopper', 4),
                                       ('humanoid_CMU', 10), ('cmu_2019_position_floor', 6), ('quadruped', 4), ('stacker', 10),
                                       ('soccer_2v2_boxhead', 5)])
def test_fp32_kernel_teacher_forced_on_more_domains(name, nsub):
  """The production (fp32) kernel on the other domains, restarted from the oracle's state at every
  env-step (random, partly interpenetrating joint configurations; up to 15 substeps per env-step):
  median error of one env-step <= 1e-6, at least 98 % of the (env, step) samples <= 5e-5.  The
  rest are contact on/off decisions that fall differently in fp32 (dist within rounding of the
  margin) -- the fp64 kernel tracks the same runs to 1e-14 (test_more_domains_rollout_parity)."""
  from dm_control_amd.batch import BatchedPhysics
  from dm_control_amd.suite import common
  from oracle import oracle
  if name.startswith('swimmer'):
    from dm_control_amd.suite import swimmer
    m = mc.compile_xml(swimmer._make_model(int(name[7:])))
  elif name == 'manipulator':
    from dm_control_amd.suite import manipulator
    m = mc.compile_xml(manipulator.make_model(False, True)[0])
  else:
    m = mc.compile_xml(common.read_model(name + '.xml'))
  NE = 16
  rs = np.random.RandomState(11)
  q = np.tile(m.qpos0, (NE, 1))
  v = np.zeros((NE, m.nv))
  if name == 'cmu_2019_position_floor':
    # BASELINE config 4 physics: start upright with perturbed joints (qpos0 is the upright pose)
    q[:, 7:] += rs.uniform(-.15, .15, (NE, m.nq - 7))
  if name == 'soccer_2v2_boxhead':
    # BASELINE config 5 physics: players spread around their kick-off spots, ball somewhere in midfield
    from dm_control_amd.composer.tasks import soccer
    adr = soccer.addresses(m)
    q = np.tile(soccer.kickoff_qpos(m), (NE, 1))
    q[:, [a for xy in adr['players'] for a in xy]] += rs.uniform(-6, 6, (NE, 8))
    q[:, adr['ball_q']:adr['ball_q'] + 2] += rs.uniform(-8, 8, (NE, 2))
    q[:, [qy + 1 for _, qy in adr['players']]] = 0.01      # root_z: at 0 the wheels touch the pitch at exactly dist = 0, an fp32 coin flip
  if name in ('manipulator', 'humanoid_CMU', 'quadruped', 'stacker'):
    # stiff (solref 5 ms), gram-scale fingertips: interpenetrating starts are ill-conditioned beyond
    # fp32; use the task's own collision-free start states (manipulator.py:183-239, humanoid_CMU.py:137-145)
    from dm_control_amd import suite
    env = suite.load(name, dict(manipulator='insert_ball', quadruped='fetch', stacker='stack_4').get(name, 'stand'), task_kwargs=dict(random=5),
                     physics_kwargs=dict(batch_size=NE))
    env.reset()
    q, v = np.array(env.physics.data.qpos), np.array(env.physics.data.qvel)
    m = env.physics.model
    env.physics.free()
  elif name not in ('cmu_2019_position_floor', 'soccer_2v2_boxhead'):
    for j in range(m.njnt):
      a = m.jnt_qposadr[j]
      if m.jnt_type[j] == 3 and m.jnt_limited[j]:
        q[:, a] = rs.uniform(m.jnt_range[j][0], m.jnt_range[j][1], NE)
  refs = []
  for e in range(NE):
    o = _oracle(m)
    o.qpos[:] = q[e]
    o.qvel[:] = v[e]
    o.forward()
    refs.append(o)
  b = BatchedPhysics(m, NE, **dict(common.DEFAULT_CAPS.get(name, {}), precision=32))
  errs = []
  for t in range(40):
    a = rs.uniform(-1, 1, (NE, m.nu))
    b.set('qpos', np.stack([o.qpos for o in refs]))
    b.set('qvel', np.stack([o.qvel for o in refs]))
    b.set('qacc_warmstart', np.stack([o.qacc_warmstart for o in refs]))
    if m.na:
      b.set('act', np.stack([o.act for o in refs]))
    b.set_control(a)
    b.step(nsub)
    oracle.rollout_legacy(refs, a[None], nsub=nsub)
    qo = np.stack([o.qpos for o in refs])
    errs.append(np.abs(b.get('qpos') - qo).max(axis=1) / np.maximum(1.0, np.abs(qo).max(axis=1)))
  errs = np.concatenate(errs)
  assert np.median(errs) <= 1e-6, np.median(errs)
  # config 4 (62 dofs, servo gains up to 150 against 0.01 armature, 6 substeps, noslip): the error is a
  # continuous rounding tail, not contact flips -- 95 % within 5e-5 and nothing beyond 1e-3
  # stacker (box piles, 10 substeps): box-box manifolds are discrete decisions (face vs edge axis, which clipped
  # points survive); in fp32 a few per cent of the env-steps take another branch -- median 6e-8, tail below 5e-3
  frac = 0.95 if name in ('cmu_2019_position_floor', 'stacker') else 0.98
  assert (errs <= 5e-5).mean() >= frac, (errs <= 5e-5).mean()
  if name in ('cmu_2019_position_floor', 'stacker'):
    assert errs.max() <= (1e-3 if name == 'cmu_2019_position_floor' else 5e-3), errs.max()
  assert not b.get('warning').any()
  b.close()


@pytest.mark.parametrize('domain,task', [('walker', 'run'), ('walker', 'stand'), ('hopper', 'hop'), ('hopper', 'stand'),
                                         ('quadruped', 'walk'), ('quadruped', 'run')])
def test_torch_env_matches_host_task(domain, task):
  """Device-resident walker / hopper: observations and rewards equal the host task evaluated on the
  same state (the host Physics is fed the device env's qpos / qvel / ctrl)."""
  import torch
  from dm_control_amd import suite
  from dm_control_amd.suite import torch_env
  B = 24
  dev = torch_env.make(domain, task, B, precision=64, seed=3)
  host = suite.load(domain, task, task_kwargs=dict(random=0), physics_kwargs=dict(batch_size=B, precision=64))
  host.reset()
  g = torch.Generator(device='cuda').manual_seed(1)
  for t in range(6):
    a = torch.rand((B, dev.model.nu), device='cuda', generator=g, dtype=torch.float64) * 2 - 1
    q_before, v_before = dev.physics.get('qpos'), dev.physics.get('qvel')
    w_before = dev.physics.get('qacc_warmstart')
    act_before = dev.physics.get('act')
    obs, rew, done = dev.step(a)
    # replay the same env-step on the host-facade physics from the same state
    hp = host.physics
    hp.data.qpos = q_before; hp.data.qvel = v_before; hp.data.qacc_warmstart = w_before
    if dev.model.na:
      hp.data.act = act_before
    hp.forward()
    hp.data.qacc_warmstart = w_before
    host.task.before_step(a.cpu().numpy(), hp)
    hp.step(dev.n_sub_steps)
    want_obs = np.concatenate([np.asarray(v).reshape(B, -1) for v in host.task.get_observation(hp).values()], axis=1)
    np.testing.assert_allclose(obs.cpu().numpy(), want_obs, rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(rew.cpu().numpy(), host.task.get_reward(hp), rtol=1e-7, atol=1e-9)
  dev.close(); host.physics.free()


@pytest.mark.parametrize('name,nsub,caps', [('cmu_2019_position_floor', 6, dict(nconmax=48)), ('soccer_2v2_boxhead', 5, dict(nconmax=24)),
                                            ('humanoid_CMU', 10, dict(nconmax=96))])
def test_baseline_62dof_and_soccer_models_fp64_open_loop(name, nsub, caps):
  """BASELINE configs 4 / 5 (and the suite's humanoid_CMU) on the fp64 instantiation of the kernel, OPEN LOOP against
  the oracle, with the production contact caps: since the contact rows, sparse M and cold tables moved to global
  memory the fp64 scratch of the 62-dof models fits twice per CU, so these configs have the same fp64 GPU parity as
  the small ones."""
  from dm_control_amd import mjcf_compiler as mc
  from dm_control_amd.batch import BatchedPhysics
  from dm_control_amd.suite import common
  from oracle.oracle import OraclePhysics, OracleModel
  m = mc.compile_xml(common.read_model(name + '.xml'))
  B, T = 6, 25
  rs = np.random.RandomState(11)
  q = np.tile(m.qpos0, (B, 1))
  if name.startswith('soccer'):
    from dm_control_amd.composer.tasks import soccer
    adr = soccer.addresses(m)
    q = np.tile(soccer.kickoff_qpos(m), (B, 1))
    q[:, [a for xy in adr['players'] for a in xy]] += rs.uniform(-8, 8, (B, 8))
    q[:, adr['ball_q']:adr['ball_q'] + 2] += rs.uniform(-15, 15, (B, 2))
  else:
    q[:, 7:] += rs.uniform(-0.15, 0.15, (B, m.nq - 7))
    q[:, 2] -= 0.25 if name == 'humanoid_CMU' else 0.0
  b = BatchedPhysics(m, B, precision=64, **caps)
  assert b.info()['precision'] == 64
  b.set('qpos', q)
  om = OracleModel(m)
  refs = [OraclePhysics(om) for _ in range(B)]
  for e, o in enumerate(refs):
    o.qpos[:] = q[e]
    o.forward()
  worst = 0.0
  for t in range(T):
    c = rs.uniform(-1, 1, (B, m.nu))
    b.set_control(c)
    b.step(nsub)
    for e, o in enumerate(refs):
      o.ctrl[:] = c[e]
      o.step(nsub)
    qo = np.stack([o.qpos for o in refs])
    worst = max(worst, float((np.abs(b.get('qpos') - qo).max(axis=1) / np.maximum(1.0, np.abs(qo).max(axis=1))).max()))
  assert worst < 1e-8, worst
  assert b.get('ncon').max() > 0 and not b.get('warning').any()
  b.close()


@pytest.mark.parametrize('cfgid', [4, 5])
def test_baseline_62dof_and_soccer_fp32_error_of_one_physics_step(cfgid):
  """north_star tolerance (1e-4 rel qpos) for the fp32 kernel on BASELINE configs 4 / 5, 64 environments x 50 env-steps:
  the GPU state is overwritten by the oracle's before EVERY physics step (legacy Physics.step(1)), so each of the
  64 x 50 x n_sub_steps comparisons is the arithmetic error of one mj_step from identical state.  (Forced only every
  env-step, 0.2 % of the env-steps exceed 1e-4 -- bench.py `parity.teacher-forced.per_step`: a contact that fp32 and
  fp64 activate one physics step apart changes the following substeps; the per-physics-step figure has no such tail.)
  Steps on which the two disagree about a contact that is JUST TOUCHING (|dist| below fp32 resolution; margin 0) are
  identified by comparing the contact sets at the forced state, counted and excluded, as in
  test_gpu_parity._teacher_forced_replay: MuJoCo's dynamics are discontinuous there.  Config 5 starts that way (the
  players' feet rest exactly on the pitch: dist = 0 in fp64, -1e-7 in fp32)."""
  import os
  import sys
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import bench
  from dm_control_amd.batch import BatchedPhysics
  from dm_control_amd.suite import common
  cfg = bench.CONFIGS[cfgid]
  nsub = cfg['nsub']
  m = bench.load_model(cfg['asset'])
  caps = dict(common.DEFAULT_CAPS.get(cfg['asset'], {}))
  caps.pop('precision', None)
  NE, T = 64, 50
  q0 = bench.initial_qpos(cfg, m, NE, seed0=0)
  refs = bench.make_oracles(m, q0, step1=False)
  for p in refs:
    p.forward()
  g = BatchedPhysics(m, NE, precision=32, **caps)
  rs = np.random.RandomState(77)
  nth = os.cpu_count() or 1
  errs = []
  events = []
  for t in range(T):
    a = rs.uniform(-1, 1, (NE, m.nu)).astype(np.float32).astype(np.float64)
    g.set_control(a)
    for k in range(nsub):
      g.set('qpos', np.stack([p.qpos for p in refs])); g.set('qvel', np.stack([p.qvel for p in refs]))
      g.forward()      # the contact set the fp32 kernel sees at the oracle's state
      ncon, dist, g1, g2 = g.get('ncon')[:, 0], g.get('contact_dist'), g.get('contact_geom1'), g.get('contact_geom2')
      edge = np.zeros(NE, bool)
      for e, p in enumerate(refs):
        if int(ncon[e]) == p.ncon:
          continue
        mine = {(int(g1[e, c]), int(g2[e, c])): float(dist[e, c]) for c in range(int(ncon[e]))}
        theirs = {(cc['geom1'], cc['geom2']): cc['dist'] for cc in (p.contact(c) for c in range(p.ncon))}
        only = [d for kk, d in mine.items() if kk not in theirs] + [d for kk, d in theirs.items() if kk not in mine]
        # margin = 0: a contact exists iff dist < 0; positions reach ~30 m on the pitch (fp32 ulp 2e-6)
        assert only and all(abs(d) < 1e-5 for d in only), ('contact sets differ beyond rounding', e, t, k, only)
        edge[e] = True
        events.append((e, t, k, only[0]))
      g.set('qacc_warmstart', np.stack([p.qacc_warmstart for p in refs]))      # mj_forward left its own solution there
      g.step(1)
      bench.threaded_rollout(refs, a[None], 1, nth)
      errs.append(np.where(edge, 0.0, bench.rel_err(g.get('qpos'), np.stack([p.qpos for p in refs]))))
  e = np.concatenate(errs)
  print('measured: config %d fp32 one-physics-step error over %d steps: median %.2e p99 %.2e max %.2e; %d steps excluded '
        'for a just-touching contact decided by the last bit: %s' % (cfgid, e.size, np.median(e), np.percentile(e, 99), e.max(), len(events), events[:6]))
  assert e.size == NE * T * nsub
  assert np.median(e) < 1e-6, np.median(e)
  assert e.max() <= 1e-4, (e.max(), np.sort(e)[-5:])
  assert len(events) <= 0.01 * e.size + NE, len(events)      # config 5 starts with every foot resting exactly on the pitch: the first step of each environment
  assert max(p.ncon for p in refs) > 0 and not g.get('warning').any()
  g.close()


@pytest.mark.parametrize('name,nsub,B', [('humanoid', 5, 4096), ('cmu_2019_position_floor', 6, 2048)])
def test_work_queue_and_schedule_do_not_change_results(name, nsub, B, monkeypatch):
  """A batch larger than the chip holds runs a resident-only grid whose waves claim environments from a device queue,
  longest first (include/dmc_batch.h: work_queue), and -- round 6 -- hands every environment's env-step out in PIECES of
  physics steps, round by round (StepIO::slices: the state travels through the state arrays between the pieces, which
  may run on different waves, CUs and XCDs).  Which wave steps an environment, and when, must not matter: the
  trajectories equal those of the static one-workgroup-per-4-environments grid bit for bit."""
  from dm_control_amd import mjcf_compiler as mc
  from dm_control_amd.batch import BatchedPhysics
  from dm_control_amd.suite import common
  m = mc.compile_xml(common.read_model(name + '.xml'))
  caps = dict(common.DEFAULT_CAPS.get(name, {}))
  caps['precision'] = 32
  rs = np.random.RandomState(3)
  q = np.tile(m.qpos0, (B, 1))
  q[:, 7:] += rs.uniform(-0.3, 0.3, (B, m.nq - 7))
  q[:B // 8, 2] -= 0.6          # some start in the ground: many contacts, long steps
  acts = rs.uniform(-1, 1, (6, B, m.nu))
  out = {}
  for mode, env in (('queue', {}), ('index_order', {'DMC_NO_LPT': '1'}), ('static', {'DMC_NO_QUEUE': '1'}),
                    ('whole_items', {'DMC_SLICES': '1'}), ('two_pieces', {'DMC_SLICES': '2'})):
    for k in ('DMC_NO_LPT', 'DMC_NO_QUEUE', 'DMC_SLICES'):
      monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    b = BatchedPhysics(m, B, **caps)
    assert b.info()['work_queue'] == (0 if mode == 'static' else 1), b.info()
    b.set('qpos', q)
    for a in acts:
      b.set_control(a)
      b.step(nsub)
    out[mode] = (b.get('qpos'), b.get('qvel'), b.get('sensordata'), b.get('ncon'), b.get('warning'), b.get('qacc_warmstart'),
                 b.get('time'), b.get('nefc'), b.get('solver_iter'), b.get('xpos'))
    b.close()
  for mode in ('index_order', 'static', 'whole_items', 'two_pieces'):
    for x, y in zip(out['queue'], out[mode]):
      np.testing.assert_array_equal(x, y, err_msg=mode)
  assert out['queue'][3].max() > 8


def test_sliced_items_with_probe_forward_after_and_launch_overrides(monkeypatch):
  """Sliced items (StepIO::slices) under everything a device environment asks of a step launch: the substep probe (one
  geom's position after every physics step), legacy_step 2 (the launch ends with mj_forward at the new state), per-env
  launch overrides (env_mode 1: mj_forward without actuation instead, 2: untouched) and launches of different nstep on
  one batch.  Pieces against whole items (DMC_SLICES=1): bit for bit."""
  import torch
  from dm_control_amd import mjcf_compiler as mc
  from dm_control_amd.batch import BatchedPhysics
  from dm_control_amd.suite import common
  m = mc.compile_xml(common.read_model('humanoid.xml'))
  caps = dict(common.DEFAULT_CAPS.get('humanoid', {})); caps['precision'] = 32
  B = 4096
  rs = np.random.RandomState(11)
  q = np.tile(m.qpos0, (B, 1))
  q[:, 7:] += rs.uniform(-0.3, 0.3, (B, m.nq - 7))
  q[:B // 8, 2] -= 0.6
  acts = rs.uniform(-1, 1, (4, B, m.nu))
  em = np.zeros((B, 1), np.int32); em[5::7] = 1; em[3::11] = 2
  g = m.name2id('left_left_foot', 'geom')
  out = {}
  for mode in ('pieces', 'whole'):
    monkeypatch.delenv('DMC_SLICES', raising=False)
    if mode == 'whole': monkeypatch.setenv('DMC_SLICES', '1')
    b = BatchedPhysics(m, B, **caps)
    assert b.info()['work_queue'] == 1
    probe = torch.zeros((5, 3, B), dtype=torch.float32, device='cuda')
    b.set_step_probe(g, probe.data_ptr(), 5)
    b.set('qpos', q)
    res = []
    for t, a in enumerate(acts):
      b.set_control(a)
      b.set('env_mode', em if t == 2 else np.zeros((B, 1), np.int32))
      b.step(5 if t != 1 else 3, forward_after=(t % 2 == 0))
      torch.cuda.synchronize()
      res += [b.get(n) for n in ('qpos', 'qvel', 'qacc_warmstart', 'sensordata', 'time', 'ncon', 'warning')] + [probe.cpu().numpy().copy()]
    out[mode] = res
    b.close()
  for x, y in zip(out['pieces'], out['whole']):
    np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize('name,flags', [('humanoid', 7), ('cheetah', 1), ('acrobot', 7), ('quadruped', 4 | 8), ('ball_xml', 7)])
def test_device_joint_randomizer_matches_the_numpy_mirror(name, flags):
  """dmc_batch_randomize_joints (suite/utils/randomizers.py:35-88 on the device, Philox4x32-10 per (env, draw, joint))
  against its numpy restatement tests/philox_mirror.py, whose generator is pinned on the published known answers: same
  values, masked environments untouched, draw counters advanced for the drawn ones only."""
  import torch
  import philox_mirror as pm
  from dm_control_amd.batch import BatchedPhysics
  from dm_control_amd.suite import common
  if name == 'ball_xml':
    m = mc.compile_xml("""<mujoco><worldbody><body><joint type='ball'/><geom size='.1'/><body pos='0 0 .3'>
        <joint type='hinge' axis='0 1 0'/><geom size='.1'/></body></body></worldbody></mujoco>""")
  else:
    m = mc.compile_xml(common.read_model(name + '.xml'))
  B = 70
  b = BatchedPhysics(m, B, precision=64)
  draw = torch.zeros(B, dtype=torch.int32, device='cuda')
  want = np.tile(m.qpos0, (B, 1)); wdraw = np.zeros(B, int)
  for rnd, mask in enumerate([None, np.arange(B) % 3 == 0, np.arange(B) % 2 == 1]):
    mt = None if mask is None else torch.from_numpy(mask.astype(np.int32)).cuda()
    b.randomize_joints(1234567890123, draw.data_ptr(), None if mt is None else mt.data_ptr(), flags)
    b.sync()
    pm.randomize_joints(m, want, 1234567890123, wdraw, mask, flags)
    np.testing.assert_allclose(b.get('qpos'), want, rtol=0, atol=1e-13)
    np.testing.assert_array_equal(draw.cpu().numpy(), wdraw)
  assert (want != np.tile(m.qpos0, (B, 1))).any()
  b.close()


@pytest.mark.parametrize('domain,task', [('humanoid', 'stand'), ('cheetah', 'run'), ('walker', 'walk'), ('quadruped', 'walk')])
def test_torch_env_draws_a_fresh_start_state_every_episode(domain, task):
  """device tasks re-initialise with a NEW draw per episode (no finite pool): two resets give every
  environment two different start states, humanoids start without contacts (suite/humanoid.py:160-165 rejection),
  cheetahs settled with time = 0 (suite/cheetah.py:63-76), and a reset of some environments leaves the others
  bit-identical."""
  import torch
  from dm_control_amd.suite import torch_env
  B = 40
  env = torch_env.make(domain, task, B, precision=32, seed=5)
  m = env.model
  q1 = env.qpos.clone()
  env.reset()
  q2 = env.qpos.clone()
  hinge_rows = [int(m.jnt_qposadr[j]) for j in range(m.njnt) if m.jnt_type[j] == 3 and (m.jnt_limited[j] or domain == 'walker')]
  if domain == 'quadruped':
    assert bool((q1[3:7] != q2[3:7]).any(dim=0).all())          # a new orientation per episode
    np.testing.assert_allclose(torch.linalg.norm(q2[3:7], dim=0).cpu().numpy(), 1, atol=1e-6)
  else:
    assert hinge_rows and bool((q1[hinge_rows] != q2[hinge_rows]).any(dim=0).all())
  assert len({tuple(c) for c in q2.T.cpu().numpy().round(6)}) == B       # and a different one per environment
  if domain in ('humanoid', 'quadruped'):
    assert int(env.ncon.max()) == 0 and env.reset_rounds >= 1
  if domain != 'cheetah':
    for j in range(m.njnt):
      if m.jnt_limited[j] and m.jnt_type[j] in (2, 3) and domain != 'quadruped':
        a = int(m.jnt_qposadr[j])
        assert float(q2[a].min()) >= m.jnt_range[j][0] - 1e-6 and float(q2[a].max()) <= m.jnt_range[j][1] + 1e-6
  else:
    assert float(env.qvel.abs().max()) < 5.0 and float(env.time.max()) == 0.0     # settled for 200 steps, clock reset
  # partial reset: the others do not move
  mask = torch.arange(B, device='cuda') % 4 == 0
  before_q, before_v, before_w = env.qpos.clone(), env.qvel.clone(), env.warm.clone()
  env.reset(mask)
  keep = ~mask
  assert torch.equal(env.qpos[:, keep], before_q[:, keep]) and torch.equal(env.qvel[:, keep], before_v[:, keep])
  assert torch.equal(env.warm[:, keep], before_w[:, keep])
  assert bool((env.qpos[:, mask] != before_q[:, mask]).any(dim=0).all())
  assert int(env._draw.min()) >= 2 and int(env._draw[mask].min()) >= 3
  env.close()


def test_collision_filter_bits_rewritten_at_run_time_on_the_device():
  """geom_contype / geom_conaffinity writes (composer/initializers/prop_initializer.py:138-160): the facade rebuilds the
  device batch from the edited model and carries the state over; the continuation equals that of a model compiled with
  the bits from the start (tests/test_facade_cpu.py holds the scenario)."""
  from test_facade_cpu import check_collision_filter_edits
  from dm_control_amd import physics as pl
  check_collision_filter_edits(pl.Physics.from_xml_string, atol=1e-12)


def test_tendon_length_and_velocity_on_the_device():
  """data.ten_length / ten_velocity (locomotion/walkers/rodent.py:279-285): derived by the facade from the device's
  qpos / qvel / site_xpos / cvel; equal to the oracle's mj_tendon and ten_J qvel."""
  from test_facade_cpu import check_tendon_length_and_velocity
  from dm_control_amd import physics as pl
  check_tendon_length_and_velocity(pl.Physics.from_xml_string, 1e-10)

"""Batched contact wrenches on the GPU: the biped of tests/contact_wrench_cases.py (pyramidal and elliptic cones, both
precisions) against the numpy twin evaluated on the device's OWN contact arrays, the fp64 kernels against the host build of
the same csrc/con_core.h bit for bit, end to end against the oracle, the resting box's weight, refresh(), determinism, a
second stream, graph capture, the refusals and suite/contact_forces.wrap.  The bounds are the CPU tier's
(tests/contact_wrench_cases.py)."""
import os

import numpy as np
import pytest

import con_emu_lib as emu
import contact_wrench_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = cc.B_GPU      # one full wave plus a ragged tail
REAL = ('wrench', 'force', 'torque', 'normal', 'dist')


def make_batch(model, precision, batch_size, **kw):
  from dm_control_amd.batch import BatchedPhysics
  return BatchedPhysics(model, batch_size, precision=precision, **kw)


def fixture_batch(precision, cone='pyramidal', batch_size=B, forward=True):
  """Environment e holds state e % 16; nconmax is the largest ncon among the states."""
  m = cc.model(cone)
  q, v = cc.states(cone)
  idx = np.arange(batch_size) % cc.NSTATE
  b = make_batch(m, precision, batch_size, nconmax=cc.nconmax(cone))
  assert b.info()['nconmax'] == cc.nconmax(cone)
  b.set('qpos', q[idx])
  b.set('qvel', v[idx])
  if forward:
    b.forward()
    b.sync()
  return b


def device_arrays(b):
  """What the unit reads, as the device holds it, in the layout of contact_wrench_cases.arrays (fp64 numpy)."""
  import torch
  torch.cuda.synchronize()
  n, nb = b.batch_size, b.model.nbody
  K = b.info()['nconmax']
  g = lambda name, *s: np.asarray(b.get(name)).reshape((n,) + s)
  return dict(ncon=g('ncon').astype(np.int32), geom1=g('contact_geom1', K).astype(np.int32), geom2=g('contact_geom2', K).astype(np.int32),
              dist=g('contact_dist', K), pos=g('contact_pos', K, 3), frame=g('contact_frame', K, 3, 3), force=g('contact_force', K, 6),
              xpos=g('xpos', nb, 3), xipos=g('xipos', nb, 3), xmat=g('xmat', nb, 3, 3))


def read_all(bc, local=None):
  import torch
  r = dict(bc.net_all(local=local), wrench=bc.wrench())
  torch.cuda.synchronize()
  return {k: v.cpu().numpy().astype(np.int32 if k == 'count' else np.float64) for k, v in r.items()}


def bound(prec, key):
  return cc.F64_TOL if prec == 64 else cc.F32_TOL[key]


@pytest.mark.parametrize('cone', cc.CONES)
@pytest.mark.parametrize('prec', [64, 32])
def test_unit_against_the_twin_on_the_devices_own_contacts(prec, cone):
  import torch
  from dm_control_amd import batch as batch_lib
  from dm_control_amd import contacts
  b = fixture_batch(prec, cone)
  m = b.model
  a = device_arrays(b)
  assert not b.get('warning').any()
  worst = dict.fromkeys(REAL, 0.0)
  for targets, about, local in ((cc.TARGETS, 'com', False), (cc.TARGETS, 'origin', True), (cc.targets64(m), 'world', False),
                                (cc.TARGETS[4:5], 'com', True)):
    bc = contacts.BatchContacts(b, targets, about=about, local=local)
    info = bc.info()
    assert (info['B'], info['precision'], info['ntarget'], info['nconmax'], info['block']) == (B, prec, len(targets), cc.nconmax(cone), 64)
    assert bc.output_mask == batch_lib.OUT['contact'] | {'com': batch_lib.OUT['xipos'], 'origin': batch_lib.OUT['xpos'], 'world': 0}[about] | (
        batch_lib.OUT['xmat'] if local else 0)
    got, ref = read_all(bc), cc.twin_all(m, a, targets, about, local)
    r = bc.net_all()
    assert r['force'].dtype == (torch.float64 if prec == 64 else torch.float32) and r['count'].dtype == torch.int32
    assert tuple(r['force'].shape) == (B, len(targets), 3) and tuple(r['dist'].shape) == (B, len(targets)) and r['torque'].is_contiguous()
    for k in REAL:
      err = cc.rel_error(got[k], ref[k])
      worst[k] = max(worst[k], err)
      assert err <= bound(prec, k), (about, local, k, err)
    np.testing.assert_array_equal(got['count'], ref['count'])
    if prec == 64:      # the same header on the host, fed the device's own arrays: equal bits
      host = emu.run(64, a, bc.tables, m.ngeom, m.nbody, local)
      for k in REAL + ('count',):
        np.testing.assert_array_equal(got[k], host[k])
    # the single-output calls are the same launch with fewer pointers
    assert torch.equal(bc.normal(), r['normal']) and torch.equal(bc.count(), r['count']) and torch.equal(bc.dist(), r['dist'])
    f, t = bc.net()
    assert torch.equal(f, r['force']) and torch.equal(t, r['torque'])
    bc.close()
  print('fp%d %s kernels worst |x - twin| / max(1, |x|max): %s' % (prec, cone, ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
  assert a['ncon'].max() == cc.nconmax(cone) and a['ncon'].min() == 0
  b.close()


@pytest.mark.parametrize('prec', [64, 32])
def test_one_environment_and_every_element_written(prec):
  import torch
  from dm_control_amd import contacts
  m = cc.model('elliptic')
  q, v = cc.states('elliptic')
  full = [r['ncon'] for r in cc.references('elliptic')].index(cc.nconmax('elliptic'))
  b = make_batch(m, prec, 1, nconmax=cc.nconmax('elliptic'))
  b.set('qpos', q[full:full + 1])
  b.set('qvel', v[full:full + 1])
  b.forward()
  b.sync()
  bc = contacts.BatchContacts(b, cc.TARGETS[:1])      # B = 1, T = 1
  a = device_arrays(b)
  got, ref = read_all(bc), cc.twin_all(m, a, cc.TARGETS[:1])
  for k in REAL:
    assert cc.rel_error(got[k], ref[k]) <= bound(prec, k)
  assert got['count'].tolist() == ref['count'].tolist() and got['count'][0, 0] >= 4
  bc.close()
  b.close()
  # out= tensors full of NaN / -1: nothing may remain; environments without a contact read exact zeros and +inf
  b = fixture_batch(prec, 'pyramidal')
  bc = contacts.BatchContacts(b, cc.TARGETS)
  _, dev, dt = bc._torch()
  T, K = len(cc.TARGETS), cc.nconmax('pyramidal')
  nan = lambda *s: torch.full(s, float('nan'), dtype=dt, device=dev)
  out = dict(force=nan(B, T, 3), torque=nan(B, T, 3), normal=nan(B, T), dist=nan(B, T), count=torch.full((B, T), -1, dtype=torch.int32, device=dev))
  w = nan(B, K, 6)
  r = bc.net_all(out=out)
  assert bc.wrench(out=w) is w and all(r[k] is out[k] for k in out)
  torch.cuda.synchronize()
  assert not any(bool(torch.isnan(t).any()) for t in (w, out['force'], out['torque'], out['normal'], out['dist'])) and int(out['count'].min()) >= 0
  ncon = torch.as_tensor(b.get('ncon')[:, 0], device=dev)
  empty = ncon == 0
  assert int(empty.sum()) >= 2 * (B // cc.NSTATE)
  assert not bool(out['force'][empty].any()) and not bool(out['torque'][empty].any()) and not bool(w[empty].any()) and not bool(out['count'][empty].any())
  assert bool(torch.all(out['dist'][empty] == float('inf'))) and bool(torch.all((out['dist'] == float('inf')) == (out['count'] == 0)))
  past = torch.arange(K, device=dev)[None, :] >= ncon[:, None]
  assert not bool(w[past].any()) and bool(w[~past].any()) and float(out['normal'].min()) >= 0
  bc.close()
  b.close()


@pytest.mark.parametrize('prec', [64, 32])
def test_end_to_end_against_the_oracle(prec):
  """forward() at the uploaded fixture states against the oracle's contact list (R1) and cfrc_ext (R2): the parity of the
  device's SOLVER, not of this unit.  Measured on an MI355X (worst error relative to max(1, |reference|max), both cones):
  see contact_wrench_cases.E2E_MEASURED; the bound is 4 x that.  count must be equal exactly."""
  from dm_control_amd import contacts
  worst = dict.fromkeys(REAL[1:] + ('cfrc_force', 'cfrc_torque'), 0.0)
  for cone in cc.CONES:
    b = fixture_batch(prec, cone)
    m, refs = b.model, cc.references(cone)
    idx = np.arange(B) % cc.NSTATE
    bc = contacts.BatchContacts(b, cc.TARGETS)
    got = read_all(bc)
    ref = cc.twin_all(m, cc.arrays(refs, cc.nconmax(cone)), cc.TARGETS)
    np.testing.assert_array_equal(got['count'], ref['count'][idx])
    np.testing.assert_array_equal(b.get('ncon')[:, 0], np.array([r['ncon'] for r in refs])[idx])
    for k in REAL[1:]:
      worst[k] = max(worst[k], cc.rel_error(got[k], ref[k][idx]))
    bc.close()
    bodies = contacts.BatchContacts(b, [t for t, _ in cc.BODY_TARGETS])
    gb = read_all(bodies)
    for t, (_, body) in enumerate(cc.BODY_TARGETS):
      want = [cc.cfrc_reference(m, r, body) for r in refs]
      f, tq = np.array([x[0] for x in want])[idx], np.array([x[1] for x in want])[idx]
      worst['cfrc_force'] = max(worst['cfrc_force'], cc.rel_error(gb['force'][:, t], f))
      worst['cfrc_torque'] = max(worst['cfrc_torque'], cc.rel_error(gb['torque'][:, t], tq))
    bodies.close()
    b.close()
  print('fp%d end to end against the oracle, worst error per output: %s' % (prec, ', '.join('%s %.3e' % kv for kv in sorted(worst.items()))))
  measured = cc.E2E_MEASURED[prec]
  assert measured is not None, 'contact_wrench_cases.E2E_MEASURED holds no measurement for fp%d' % prec
  for k, v in worst.items():
    assert v <= 4 * measured[k], (k, v)


@pytest.mark.parametrize('prec', [64, 32])
def test_settled_box_carries_its_weight(prec):
  """R3 on the device."""
  from dm_control_amd import contacts
  b = make_batch(cc.model('box'), prec, 3)
  b.step(2000, forward_after=True)
  b.sync()
  bc = contacts.BatchContacts(b, ['box', dict(geom='floor')])
  got = read_all(bc)
  weight = cc.BOX_MASS * 9.81
  print('fp%d settled box: normal %s, weight %.9g' % (prec, got['normal'][:, 0], weight))
  assert got['count'].tolist() == [[4, 4]] * 3
  assert np.abs(got['normal'] - weight).max() <= cc.WEIGHT_TOL[prec] * weight
  assert np.abs(got['force'][:, 0, 2] - weight).max() <= cc.WEIGHT_TOL[prec] * weight
  assert np.abs(got['force'][:, 1, 2] + weight).max() <= cc.WEIGHT_TOL[prec] * weight
  bc.close()
  b.close()


@pytest.mark.parametrize('prec', [64, 32])
def test_refresh_leaves_the_state_and_the_warm_start_alone(prec):
  import torch
  from dm_control_amd import contacts
  a, t1, t2 = (fixture_batch(prec, 'elliptic') for _ in range(3))
  bca, bc1 = contacts.BatchContacts(a, cc.TARGETS), contacts.BatchContacts(t1, cc.TARGETS)
  # step(forward_after=True) gives the bits of a plain legacy step followed by refresh()
  a.step(3, forward_after=True)
  for b in (t1, t2):
    b.step(3)
  t1.sync()
  state = ('qpos', 'qvel', 'time', 'qacc_warmstart', 'act')
  before = {k: t1.get(k) for k in state}
  bc1.refresh()
  ra, r1 = read_all(bca), read_all(bc1)
  for k in ra:
    np.testing.assert_array_equal(ra[k], r1[k])
  # refresh() moved neither the state nor the warm start: t2 was never refreshed
  torch.cuda.synchronize()
  for k in state:
    np.testing.assert_array_equal(t1.get(k), before[k])
    np.testing.assert_array_equal(t1.get(k), t2.get(k))
  # ... and left arrays that are consistent with each other: the twin on the device's own contacts
  arr = device_arrays(t1)
  ref = cc.twin_all(t1.model, arr, cc.TARGETS)
  for k in REAL:
    assert cc.rel_error(r1[k], ref[k]) <= bound(prec, k)
  np.testing.assert_array_equal(r1['count'], ref['count'])
  live = np.arange(arr['geom1'].shape[1])[None, :] < arr['ncon'][:, None]
  assert np.abs(arr['force'][live][:, 0]).max() > 1 and not arr['force'][~live].any()
  # the next step of the refreshed batch is the never-refreshed twin's, bit for bit
  for b in (t1, t2):
    b.step(1)
  t1.sync()
  t2.sync()
  for k in state:
    np.testing.assert_array_equal(t1.get(k), t2.get(k))
  bca.close()
  bc1.close()
  for b in (a, t1, t2):
    b.close()


def test_equal_bits_across_launches_and_on_a_second_stream():
  import torch
  from dm_control_amd import contacts
  b = fixture_batch(32, 'pyramidal', 130)
  bc = contacts.BatchContacts(b, cc.targets64(b.model), about='origin', local=True)
  r1, w1 = bc.net_all(), bc.wrench()
  bc.normal()      # other launches in between change nothing
  r2, w2 = bc.net_all(), bc.wrench()
  assert all(torch.equal(r1[k], r2[k]) for k in r1) and torch.equal(w1, w2) and bool(r1['force'].any())
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    r3, w3 = bc.net_all(stream=s), bc.wrench(stream=s)
  s.synchronize()
  assert all(torch.equal(r1[k], r3[k]) for k in r1) and torch.equal(w1, w3)
  bc.close()
  b.close()


def test_a_graph_of_forward_and_net_all_replays_after_the_state_changed():
  import torch
  from dm_control_amd import contacts
  b = fixture_batch(32, 'pyramidal', 40)
  b.wait_specialised()
  bc = contacts.BatchContacts(b, cc.TARGETS)
  _, dev, dt = bc._torch()
  T = len(cc.TARGETS)
  out = dict(force=torch.zeros(40, T, 3, dtype=dt, device=dev), torque=torch.zeros(40, T, 3, dtype=dt, device=dev),
             normal=torch.zeros(40, T, dtype=dt, device=dev), dist=torch.zeros(40, T, dtype=dt, device=dev),
             count=torch.zeros(40, T, dtype=torch.int32, device=dev))
  before = {k: v.clone() for k, v in bc.net_all().items()}
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    b.forward(stream=torch.cuda.current_stream().cuda_stream)
    bc.net_all(out=out)
  q, v = cc.states('pyramidal')
  idx = (np.arange(40) + 5) % cc.NSTATE      # other states
  b.set('qpos', q[idx])
  b.set('qvel', v[idx])
  for t in out.values():
    t.zero_()
  graph.replay()
  torch.cuda.synchronize()
  now = bc.net_all()      # (what the replayed forward left in device memory)
  torch.cuda.synchronize()
  assert not torch.equal(now['force'], before['force'])      # the state did change
  assert all(torch.equal(out[k], now[k]) for k in out)
  bc.close()
  b.close()


def test_refusals_on_the_device():
  from dm_control_amd import _native
  from dm_control_amd import batch as batch_lib
  from dm_control_amd import contacts
  b = fixture_batch(32, 'pyramidal', 8)
  bc = contacts.BatchContacts(b, cc.TARGETS)
  bc.net_all()
  b.set_output_mask(batch_lib.OUT_ALL & ~batch_lib.OUT['contact'])
  for call in (bc.net_all, bc.wrench, bc.count):
    with pytest.raises(ValueError, match='output mask'):
      call()
  b.set_output_mask(batch_lib.OUT_ALL & ~batch_lib.OUT['xipos'])
  with pytest.raises(ValueError, match='output mask'):
    bc.net()
  bc.normal()      # (reads no pose)
  b.forward()
  b.set_output_mask(batch_lib.OUT_ALL)      # asked for again, but the last launch ran without xipos: the library refuses
  with pytest.raises(_native.NativeError, match='stale'):
    bc.net()
  b.forward()
  bc.net()
  # the library validates the tables again
  import ctypes
  L = _native.lib()
  m = b.model
  body = np.zeros(65, np.int32)
  masks = np.ones((65, 2, 1), np.uint32)

  def create(T, ngeom=m.ngeom, words=1, about=0):
    tb = contacts._Tables(T, ngeom, words, about, body.ctypes.data, masks.ctypes.data)
    out = ctypes.c_void_p()
    rc = L.dmc_con_create(b._ptr, ctypes.byref(tb), ctypes.byref(out))
    assert rc != 0 and not out.value
    return L.dmc_last_error().decode()

  assert 'at most 64' in create(65) and 'at least one' in create(0) and 'not sized' in create(1, ngeom=m.ngeom + 1) and 'not sized' in create(1, words=2)
  assert 'about' in create(1, about=3)
  masks[0, 0, 0] = 0
  assert 'empty' in create(1)
  masks[0, 0, 0] = 1 << m.ngeom
  assert 'outside the model' in create(1)
  masks[0, 0, 0], body[0] = 1, m.nbody
  assert 'body id' in create(1)
  bc.close()
  b.close()


def _feet(m):
  names = m.names['geom']
  feet = [n for n in names if n and 'foot' in n and 'touch' not in n]
  ground = [n for n in names if n and ('ground' in n or 'floor' in n)]
  assert feet and ground
  return [dict(geom=f, other=ground[0]) for f in feet]


def test_contact_forces_wrap_on_a_fused_walker():
  import torch
  from dm_control_amd import contacts
  from dm_control_amd.suite import contact_forces, fused_env
  env = fused_env.make('walker', 'walk', 8)
  m = env.model if hasattr(env, 'model') else env.physics.model
  targets = _feet(m)
  wenv = contact_forces.wrap(env, targets, contact_only=True, quantity='wrench', refresh=True)
  obs = wenv.reset()
  assert tuple(obs.shape) == (8, 6 * len(targets)) and obs.dtype == env.dtype and obs.device.type == 'cuda'
  direct = contacts.BatchContacts(wenv.contacts.batch, targets)
  act = torch.zeros((8, m.nu), dtype=env.dtype, device=env.device)
  touched = pushed = False
  for _ in range(30):      # (the walker is dropped, lands on its feet and falls over under random actions)
    act.uniform_(-1, 1)
    obs, reward, done = wenv.step(act)
    f, t = direct.net()
    assert torch.equal(obs, torch.cat([f, t], dim=-1).reshape(8, -1)) and reward.shape == (8,)
    touched, pushed = touched or bool((direct.count() > 0).any()), pushed or bool((obs.abs() > 0).any())
  assert touched and pushed      # a foot was on the floor at some step
  both = contact_forces.wrap(env, targets, quantity='normal', scale='tanh')
  o2 = both.step(act)[0]
  assert set(o2) == {'state', 'contact_force'} and tuple(o2['contact_force'].shape) == (8, len(targets))
  assert torch.equal(o2['contact_force'], torch.tanh(direct.normal() / 100.0))


def test_contact_forces_wrap_on_the_composer_walker():
  import torch
  from dm_control_amd import composer
  from dm_control_amd import contacts
  from dm_control_amd.suite import contact_forces
  env = composer.make('cmu_go_to_target', 8, random_state=3)
  m = env.task.model
  targets = _feet(m)
  wenv = contact_forces.wrap(env, targets, quantity='force', refresh=False)      # the control step ends in the forward
  ts = wenv.reset()
  direct = contacts.BatchContacts(wenv.contacts.batch, targets)
  assert tuple(ts.observation['contact_force'].shape) == (8, 3 * len(targets))
  gen = torch.Generator(device='cuda').manual_seed(0)
  touched = False
  for _ in range(25):
    ts = wenv.step(torch.rand((8, m.nu), device='cuda', generator=gen) * 2 - 1)
    obs = ts.observation['contact_force']
    assert torch.equal(obs, direct.net()[0].reshape(8, -1)) and len(ts.observation) > 1
    touched = touched or (bool((direct.count() > 0).any()) and bool((obs.abs() > 0).any()))
  assert touched      # a foot was on the ground at some step
  env.close()

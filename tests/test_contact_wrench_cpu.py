"""CPU tier of the batched contact wrenches (dm_control_amd/contacts.py, csrc/con_core.h): the host build of the device
header in both real types against the numpy twin on the oracle's contact lists; the oracle's cfrc_ext, the resting box's
weight and Newton's third law as references of their own; exact zeros without contacts, every element written; `local` and
the three `about` choices; the refusals; host_data.contact_wrenches and Physics.data.contact_wrenches; the observation
wrapper on the oracle stand-in; the sanitizers on a stand-alone program."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import con_emu_lib as emu      # noqa: E402
import contact_wrench_cases as cc      # noqa: E402
from dm_control_amd import contacts      # noqa: E402
from dm_control_amd import host_data      # noqa: E402

REAL = ('wrench', 'force', 'torque', 'normal', 'dist')


@pytest.fixture(scope='module')
def world():
  """Per cone: dict(m, refs (the oracle after forward() at the 16 states), K (nconmax), a (the unit's input arrays of them))."""
  w = {}
  for cone in cc.CONES:
    m, refs = cc.model(cone), cc.references(cone)
    K = cc.nconmax(cone)
    w[cone] = dict(m=m, refs=refs, K=K, a=cc.arrays(refs, K))
  return w


def _run(w, prec, targets, about='com', local=False, a=None, **kw):
  m = w['m']
  return emu.run(prec, w['a'] if a is None else a, contacts.target_tables(m, targets, about), m.ngeom, m.nbody, local, **kw)


def test_fixture_states_hold_what_the_tests_rely_on(world):
  for cone in cc.CONES:
    s = cc.check_states(cone)
    print(cone, s)
    assert s['nconmax'] == world[cone]['K'] == 10
  m = world['pyramidal']['m']
  assert m.ngeom == 9 and m.nbody == 9 and m.nsensordata == 3
  assert len(cc.targets64(m)) == 64 and emu.caps(m.ngeom)['words'] == 1 and emu.caps(33)['words'] == 2


def test_fp64_host_build_against_the_twin(world):
  for cone in cc.CONES:
    w = world[cone]
    for targets, about, local in ((cc.TARGETS, 'com', False), (cc.TARGETS, 'origin', True), (cc.TARGETS, 'world', False),
                                  (cc.TARGETS, 'com', True), (cc.targets64(w['m']), 'com', False), (cc.TARGETS[4:5], 'origin', False)):
      got, ref = _run(w, 64, targets, about, local), cc.twin_all(w['m'], w['a'], targets, about, local)
      for k in REAL:
        assert cc.rel_error(got[k], ref[k]) <= cc.F64_TOL, (cone, about, local, k)
      np.testing.assert_array_equal(got['count'], ref['count'])
  # B = 1, the fullest state
  w = world['pyramidal']
  s = [r['ncon'] for r in w['refs']].index(w['K'])
  a1 = cc.arrays(w['refs'][s:s + 1], w['K'])
  got, ref = _run(w, 64, cc.TARGETS, a=a1), cc.twin_all(w['m'], a1, cc.TARGETS)
  for k in REAL:
    assert cc.rel_error(got[k], ref[k]) <= cc.F64_TOL
  np.testing.assert_array_equal(got['count'], ref['count'])
  assert got['count'].max() >= 4


def test_fp32_host_build_against_the_fp64_twin(world):
  worst = dict.fromkeys(REAL, 0.0)
  for cone in cc.CONES:
    w = world[cone]
    a32 = cc.round32(w['a'])
    for targets, about, local in ((cc.TARGETS, 'com', False), (cc.TARGETS, 'origin', True), (cc.TARGETS, 'world', True)):
      got, ref = _run(w, 32, targets, about, local, a=a32), cc.twin_all(w['m'], a32, targets, about, local)
      for k in REAL:
        worst[k] = max(worst[k], cc.rel_error(got[k], ref[k]))
      np.testing.assert_array_equal(got['count'], ref['count'])
  print('fp32 host build against the fp64 twin, worst error per output:', {k: '%.3e' % v for k, v in worst.items()})
  for k in REAL:
    assert worst[k] <= cc.F32_TOL[k], (k, worst[k])


def test_whole_body_targets_equal_the_oracles_cfrc_ext(world):
  """R2: independent of the twin's membership logic."""
  for cone in cc.CONES:
    w = world[cone]
    m = w['m']
    targets = [t for t, _ in cc.BODY_TARGETS]
    for about in ('com', 'origin', 'world'):
      got = _run(w, 64, targets, about)
      host = host_data.contact_wrenches(m, _getter(w['a']), targets, about)
      for s, r in enumerate(w['refs']):
        for t, (_, body) in enumerate(cc.BODY_TARGETS):
          f, tq = cc.cfrc_reference(m, r, body, about)
          for g in (got, host):
            assert np.abs(g['force'][s, t] - f).max() <= cc.F64_TOL * max(1.0, np.abs(f).max()), (cone, about, s, body)
            assert np.abs(g['torque'][s, t] - tq).max() <= cc.F64_TOL * max(1.0, np.abs(tq).max()), (cone, about, s, body)
    assert max(np.abs(r['cfrc_ext']).max() for r in w['refs']) > 10      # (the reference is not trivially zero)


def test_resting_box_normal_force_is_its_weight():
  """R3."""
  from oracle.oracle import OraclePhysics
  m = cc.model('box')
  p = OraclePhysics(m)
  p.forward()
  p.step(2000)
  ref = cc.oracle_state(m, np.array(p.qpos), np.array(p.qvel))
  assert ref['ncon'] == 4
  a = cc.arrays([ref], 4)
  weight = cc.BOX_MASS * 9.81
  for prec in (64, 32):
    got = emu.run(prec, a, contacts.target_tables(m, ['box', dict(geom='floor')]), m.ngeom, m.nbody)
    print('fp%d normal %.12g weight %.12g' % (prec, got['normal'][0, 0], weight))
    assert abs(got['normal'][0, 0] - weight) <= cc.WEIGHT_TOL[prec] * weight
    assert abs(got['force'][0, 0, 2] - weight) <= cc.WEIGHT_TOL[prec] * weight and abs(got['force'][0, 1, 2] + weight) <= cc.WEIGHT_TOL[prec] * weight
    assert got['count'].tolist() == [[4, 4]] and got['normal'][0, 1] == got['normal'][0, 0]


def test_newtons_third_law(world):
  """R4: net(S | other=O) = -net(O | other=S), and the forces over all bodies, the world included, sum to zero."""
  for cone in cc.CONES:
    w = world[cone]
    m = w['m']
    pairs = [(dict(body='foot_l'), dict(geom='floor')), (dict(body='ball'), dict(body='thigh_l', subtree=True)),
             (dict(body='torso', subtree=True), dict(body='world')), (dict(geom='ball'), dict(geom=['foot_l', 'foot_r', 'floor']))]
    targets = []
    for s, o in pairs:
      targets += [dict(s, other=o), dict(o, other=s)]
    got = _run(w, 64, targets, 'world')
    for k in range(len(pairs)):
      for key in ('force', 'torque'):
        scale = max(1.0, np.abs(got[key][:, 2*k]).max())
        assert np.abs(got[key][:, 2*k] + got[key][:, 2*k + 1]).max() <= cc.F64_TOL * scale, (cone, k, key)
      np.testing.assert_array_equal(got['count'][:, 2*k], got['count'][:, 2*k + 1])
      np.testing.assert_array_equal(got['normal'][:, 2*k], got['normal'][:, 2*k + 1])
      np.testing.assert_array_equal(got['dist'][:, 2*k], got['dist'][:, 2*k + 1])
    assert np.abs(got['force'][:, 0]).max() > 10
    everybody = _run(w, 64, [dict(body=b) for b in range(m.nbody)], 'world')
    for key in ('force', 'torque'):
      total = everybody[key].sum(axis=1)
      assert np.abs(total).max() <= cc.F64_TOL * max(1.0, np.abs(everybody[key]).max()), (cone, key)
    assert everybody['count'].sum() == 2 * sum(r['ncon'] for r in w['refs'])


def test_zeros_without_contacts_and_every_element_written(world):
  for cone in cc.CONES:
    w = world[cone]
    empty = [s for s, r in enumerate(w['refs']) if r['ncon'] == 0]
    assert empty
    for prec in (64, 32):
      for local in (False, True):
        got = _run(w, prec, cc.TARGETS, 'com', local)      # (prefilled with NaN / -1 by con_emu_lib.run)
        assert not any(np.isnan(got[k]).any() for k in REAL) and got['count'].min() >= 0
        for s in empty:
          assert not got['force'][s].any() and not got['torque'][s].any() and not got['normal'][s].any() and not got['wrench'][s].any()
          assert not got['count'][s].any() and np.all(got['dist'][s] == np.inf)
        for s, r in enumerate(w['refs']):
          assert not got['wrench'][s, r['ncon']:].any() and (got['wrench'][s].any() or not r['ncon'])
        assert np.all((got['dist'] == np.inf) == (got['count'] == 0)) and got['normal'].min() >= 0
  # stale slots past ncon are not read: garbage there changes nothing
  w = world['pyramidal']
  a = {k: v.copy() for k, v in w['a'].items()}
  for s, r in enumerate(w['refs']):
    n = r['ncon']
    a['geom1'][s, n:], a['geom2'][s, n:] = 5, 0
    for k in ('dist', 'pos', 'frame', 'force'):
      a[k][s, n:] = 7.5
  clean, dirty = _run(w, 64, cc.TARGETS), _run(w, 64, cc.TARGETS, a=a)
  for k in REAL + ('count',):
    np.testing.assert_array_equal(clean[k], dirty[k])
  # a count outside [0, nconmax] is held inside the arrays; a geom id outside the model never counts
  a = {k: v.copy() for k, v in w['a'].items()}
  full = [r['ncon'] for r in w['refs']].index(w['K'])
  a['ncon'][full] = w['K'] + 5
  a['ncon'][0] = -3
  a['geom2'][1, 0] = 1000
  got = _run(w, 64, cc.TARGETS, a=a)
  np.testing.assert_array_equal(got['force'][full], clean['force'][full])
  assert not got['force'][0].any() and got['count'][1].sum() < clean['count'][1].sum()


def test_local_frame_and_about_choices(world):
  w = world['pyramidal']
  m = w['m']
  tg = [dict(body='foot_l'), dict(geom='ball')]
  body = [m.name2id('foot_l', 'body'), m.name2id('ball', 'body')]
  got = {ab: _run(w, 64, tg, ab) for ab in ('com', 'origin', 'world')}
  loc = _run(w, 64, tg, 'com', True)
  for t, b in enumerate(body):
    R = w['a']['xmat'][:, b]
    for ab, field in (('com', 'xipos'), ('origin', 'xpos')):      # t_r = t_0 - r x f
      r = w['a'][field][:, b]
      want = got['world']['torque'][:, t] - np.cross(r, got['world']['force'][:, t])
      assert np.abs(got[ab]['torque'][:, t] - want).max() <= cc.F64_TOL * max(1.0, np.abs(want).max())
      np.testing.assert_array_equal(got[ab]['force'][:, t], got['world']['force'][:, t])
    for key in ('force', 'torque'):
      want = np.einsum('eij,ei->ej', R, got['com'][key][:, t])
      assert np.abs(loc[key][:, t] - want).max() <= cc.F64_TOL * max(1.0, np.abs(want).max())
    for key in ('normal', 'dist', 'count'):
      np.testing.assert_array_equal(loc[key], got['com'][key])
  assert np.abs(m.body_ipos[body[0]]).max() > 0.01      # xipos != xpos for the foot: the two choices differ
  assert np.abs(got['com']['torque'][:, 0] - got['origin']['torque'][:, 0]).max() > 1e-3


def _getter(a):
  names = dict(ncon='ncon', contact_geom1='geom1', contact_geom2='geom2', contact_dist='dist', contact_pos='pos', contact_frame='frame',
               contact_force='force', xpos='xpos', xipos='xipos', xmat='xmat')
  B = len(a['ncon'])
  return lambda n, *shape: np.asarray(a[names[n]]).reshape((B,) + shape)


def test_host_data_contact_wrenches(world, oracle_backend):
  for cone in cc.CONES:
    w = world[cone]
    for about, local in (('com', False), ('origin', True), ('world', False)):
      got, ref = host_data.contact_wrenches(w['m'], _getter(w['a']), cc.TARGETS, about, local), cc.twin_all(w['m'], w['a'], cc.TARGETS, about, local)
      for k in REAL[1:]:
        assert cc.rel_error(got[k], ref[k]) <= cc.F64_TOL, (cone, about, local, k)
      np.testing.assert_array_equal(got['count'], ref['count'])
      assert got['count'].dtype == np.int32
  # one environment through the Physics facade on the oracle stand-in: the settled box carries its weight
  from dm_control_amd import physics
  p = physics.Physics.from_xml_string(cc.BOX_XML)
  p.step(2000)
  warm = np.array(p.data.qacc_warmstart)
  r = p.data.contact_wrenches(['box'])
  assert r['force'].shape == (1, 3) and r['count'].tolist() == [4]
  assert abs(r['normal'][0] - cc.BOX_MASS * 9.81) <= cc.WEIGHT_TOL[64] * cc.BOX_MASS * 9.81
  np.testing.assert_array_equal(np.array(p.data.qacc_warmstart), warm)      # the query did not move the warm start


def test_refusals_are_loud(world):
  m = world['pyramidal']['m']
  with pytest.raises(TypeError, match='BatchedPhysics'):
    contacts.BatchContacts(object(), ['foot_l'])
  with pytest.raises(ValueError, match="No geom with name 'nope'"):
    contacts.target_tables(m, ['nope'])
  with pytest.raises(ValueError, match="No body with name 'nope'"):
    contacts.target_tables(m, [dict(body='foot_l', other=dict(body='nope'))])
  with pytest.raises(ValueError, match='out of range'):
    contacts.target_tables(m, [m.ngeom])
  with pytest.raises(ValueError, match='at most 64'):
    contacts.target_tables(m, ['foot_l'] * 65)
  with pytest.raises(ValueError, match='at least one target'):
    contacts.target_tables(m, [])
  with pytest.raises(ValueError, match='about must be'):
    contacts.target_tables(m, ['foot_l'], about='centre')
  for bad in (dict(site='imu'), dict(geom='ball', subtree=True), 1.5, dict(body='ball', geom='ball'), None):
    with pytest.raises(ValueError, match='expected a geom name'):
      contacts.target_tables(m, [bad])
  from dm_control_amd import mjcf_compiler as mc
  bare = mc.compile_xml('<mujoco><worldbody><geom name="g" size=".1"/><body name="bare"><joint/><inertial pos="0 0 0" mass="1" '
                        'diaginertia="1 1 1"/><body name="leaf"><geom name="l" size=".1"/></body></body></worldbody></mujoco>')
  with pytest.raises(ValueError, match='set of geoms is empty'):
    contacts.target_tables(bare, [dict(body='bare')])
  assert contacts.target_tables(bare, [dict(body='bare', subtree=True)])['masks'][0, 0, 0] == 2
  # the masks: S, O and the named body
  tb = contacts.target_tables(m, [dict(body='thigh_l', subtree=True, other='floor'), 'ball'])
  g = lambda n: m.name2id(n, 'geom')
  assert tb['masks'].shape == (2, 2, 1) and tb['masks'].dtype == np.uint32
  assert int(tb['masks'][0, 0, 0]) == sum(1 << g(n) for n in ('thigh_l', 'shin_l', 'foot_l')) and int(tb['masks'][0, 1, 0]) == 1 << g('floor')
  assert int(tb['masks'][1, 1, 0]) == (1 << m.ngeom) - 1 and tb['body'].tolist() == [m.name2id('thigh_l', 'body'), m.name2id('ball', 'body')]
  assert contacts.pack_mask(np.arange(70) % 33 == 0).tolist() == [1, 2, 4]
  # the output mask a call needs, checked before anything is launched: a stand-in for the object (no device here)
  import torch
  from dm_control_amd import batch as batch_lib
  bc = contacts.BatchContacts.__new__(contacts.BatchContacts)
  bc.batch = types.SimpleNamespace(device_id=0, precision=64, batch_size=4, output_mask=batch_lib.OUT_ALL & ~batch_lib.OUT['contact'])
  bc.about, bc.local, bc.tables, bc.nconmax = 'com', False, tb, 10
  for call in (bc.wrench, bc.net, bc.normal, bc.count, bc.dist, bc.net_all):
    with pytest.raises(ValueError, match='output mask'):
      call()
  bc.batch.output_mask = batch_lib.OUT['contact']
  for call in (bc.net, bc.net_all):      # the torque's lever arm reads xipos
    with pytest.raises(ValueError, match='output mask'):
      call()
  bc.batch.output_mask = batch_lib.OUT['contact'] | batch_lib.OUT['xipos']
  with pytest.raises(ValueError, match='output mask'):
    bc.net(local=True)      # xmat
  with pytest.raises(ValueError, match='out: expected a contiguous'):
    bc.normal(out=torch.zeros(4, 2))      # (not on the device)
  with pytest.raises(ValueError, match='2 tensors'):
    bc.net(out=[torch.zeros(1)])
  assert contacts.BatchContacts._need(bc, True, True) == batch_lib.OUT['contact'] | batch_lib.OUT['xipos'] | batch_lib.OUT['xmat']


class _HostContacts:
  """BatchContacts on the oracle stand-in: host_data.contact_wrenches as torch CPU tensors (the wrapper's logic is what is tested)."""

  def __init__(self, env, targets, about='com', local=False):
    import torch
    from dm_control_amd import batch as batch_lib
    self.batch, self.targets, self.about, self.local, self.torch = env.physics, targets, about, local, torch
    self.output_mask = batch_lib.OUT['contact'] | batch_lib.OUT['xipos']
    self.refreshed = 0

  def _all(self):
    b = self.batch
    get = lambda n, *shape: np.asarray(b.get(n)).reshape((b.batch_size,) + shape)
    return {k: self.torch.as_tensor(v) for k, v in host_data.contact_wrenches(b.model, get, self.targets, self.about, self.local).items()}

  def net(self):
    r = self._all()
    return r['force'], r['torque']

  def normal(self):
    return self._all()['normal']

  def refresh(self):
    self.refreshed += 1
    self.batch.forward()


def test_observation_wrapper_on_the_oracle_stand_in(monkeypatch, oracle_backend):
  import torch
  from dm_control_amd.suite import contact_forces
  monkeypatch.setattr(contact_forces.contacts_lib, 'BatchContacts', _HostContacts)
  m = cc.model('pyramidal')
  q, v = cc.states('pyramidal')

  class Env:
    def __init__(self):
      self.physics = oracle_backend.OracleBatch(m, 3, nconmax=10)
      self.physics.output_mask, self.masks = 0, []
      self.physics.set_output_mask = lambda mask: (self.masks.append(mask), setattr(self.physics, 'output_mask', mask))
      self.output_mask = 0

    def reset(self):
      self.physics.set('qpos', q[[1, 3, 0]])
      self.physics.set('qvel', v[[1, 3, 0]])
      self.physics.forward()
      return np.zeros((3, 2))

    def step(self, action=None):
      self.physics.step(1)
      return np.zeros((3, 2)), np.zeros(3), np.zeros(3, bool)

  targets = [dict(body='foot_l', other='floor'), dict(body='foot_r', other='floor')]
  env = contact_forces.wrap(Env(), targets, quantity='force')
  assert env.contacts.output_mask and env.env.masks == [env.contacts.output_mask] and env.env.output_mask == env.contacts.output_mask
  obs = env.reset()
  assert set(obs) == {'state', 'contact_force'} and obs['contact_force'].shape == (3, 6) and env.contacts.refreshed == 1
  refs = [cc.references('pyramidal')[s] for s in (1, 3, 0)]
  want = cc.twin_all(m, cc.arrays(refs, 10), targets)
  assert cc.rel_error(obs['contact_force'].numpy().reshape(3, 2, 3), want['force']) <= cc.F64_TOL
  assert not obs['contact_force'][2].any() and obs['contact_force'][0, 2] > 10
  out = env.step()
  assert isinstance(out, tuple) and out[0]['contact_force'].shape == (3, 6) and env.contacts.refreshed == 2
  env = contact_forces.wrap(Env(), targets, contact_only=True, quantity='normal', refresh=False)
  n = env.reset()
  assert n.shape == (3, 2) and env.contacts.refreshed == 0 and cc.rel_error(n.numpy(), want['normal']) <= cc.F64_TOL
  env = contact_forces.wrap(Env(), targets, contact_only=True, quantity='wrench', scale='tanh', scale_force=50.0, about='origin')
  wr = env.reset()
  want = cc.twin_all(m, cc.arrays(refs, 10), targets, 'origin')
  ref = np.tanh(np.concatenate([want['force'], want['torque']], axis=-1).reshape(3, 12) / 50.0)
  assert wr.shape == (3, 12) and np.abs(wr.numpy() - ref).max() <= 1e-12 and torch.all(wr.abs() < 1)
  for bad in (dict(scale='log'), dict(quantity='energy'), dict(scale='tanh', scale_force=0.0)):
    with pytest.raises(ValueError):
      contact_forces.wrap(Env(), targets, **bad)


def test_native_entry_points_validate_without_a_device():
  from dm_control_amd import build
  build.build()
  from dm_control_amd import _native
  with open(os.path.join(ROOT, 'include', 'dmc_con.h')) as f:
    declared = set(re.findall(r'\b(dmc_con_[a-z0-9_]+)\s*\(', f.read()))
  assert declared == set(_native.CON_EXPORTS)
  L = _native.lib()
  assert not [n for n in sorted(declared) if not hasattr(L, n)]
  out = ctypes.c_void_p()
  buf = (ctypes.c_double * 16)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  assert L.dmc_con_create(None, p, ctypes.byref(out)) != 0 and b'null' in L.dmc_last_error() and not out.value
  assert L.dmc_con_wrench(None, p, None) != 0 and b'null' in L.dmc_last_error()
  assert L.dmc_con_net(None, 0, p, p, p, p, p, None) != 0 and b'null' in L.dmc_last_error()
  assert L.dmc_con_warmstart(None, 0, None) != 0 and L.dmc_con_info(None, p) != 0
  L.dmc_con_destroy(None)
  units = {u[0]: u for u in build._UNITS}
  assert 'con_core.h' in units['con_kernels.hip'][2] and '-ffp-contract=off' in units['con_kernels.hip'][1]
  c = emu.caps(9)
  assert c['block'] == 64 and c['max_targets'] == contacts.MAX_TARGETS == 64 and 2 * c['max_words'] * 4 <= 65536
  for src in ('con_core.h', 'con_kernels.hip'):
    with open(os.path.join(build.CSRC, src)) as f:
      text = f.read()
    assert not re.search(r'\basm\b|__asm|atomic[A-Z_(]', text)      # plain arithmetic: no assembly, no atomic call


def test_sanitized_stand_alone_program_over_the_cases(tmp_path, world):
  """csrc/con_core.h under AddressSanitizer and UBSan: a program with its own main (tests/emu/con_sanitize.cpp), fed the
  fixture's arrays as text -- the ncon == nconmax states and T = 64 included -- in both precisions; never through Python,
  never on a GPU."""
  exe = str(tmp_path / 'con_sanitize')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                         '-Wno-unknown-pragmas', '-o', exe, os.path.join(ROOT, 'tests', 'emu', 'con_sanitize.cpp')])
  ints = lambda a: ' '.join(str(int(x)) for x in np.asarray(a).ravel())
  num = lambda a: ' '.join(repr(float(x)) for x in np.asarray(a).ravel())
  for cone, targets, about, local in (('pyramidal', cc.targets64(world['pyramidal']['m']), 'com', 1), ('elliptic', cc.TARGETS, 'origin', 0),
                                      ('elliptic', cc.TARGETS[:1], 'world', 0)):
    w = world[cone]
    m, a = w['m'], w['a']
    assert w['K'] in a['ncon']
    tb = contacts.target_tables(m, targets, about)
    T, words = tb['masks'].shape[0], tb['masks'].shape[2]
    lines = ['%d %d %d %d %d %d %d %d' % (cc.NSTATE, w['K'], m.ngeom, m.nbody, T, words, tb['about'], local),
             ints(a['ncon']), ints(a['geom1']), ints(a['geom2'])] + [num(a[k]) for k in ('dist', 'pos', 'frame', 'force', 'xpos', 'xipos', 'xmat')]
    lines += [ints(tb['body']), ints(tb['masks'])]
    res = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120, check=False)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [np.array([float(x) for x in l.split()]) for l in res.stdout.strip().split('\n')]
    n, nt = cc.NSTATE * w['K'], cc.NSTATE * T
    assert len(rows) == 2 and all(r.shape == (6*n + 9*nt,) for r in rows)
    for row, prec in zip(rows, (64, 32)):
      r = _run(w, prec, targets, about, bool(local))
      want = np.concatenate([r[k].ravel() for k in ('wrench', 'force', 'torque', 'normal', 'dist', 'count')])
      np.testing.assert_array_equal(row, want)      # (-O1 against the library's -O2, both without contraction: the same IEEE operations)

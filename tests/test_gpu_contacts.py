"""Contact-level parity of the device narrow phase with the fp64 oracle: every case of tests/contact_cases.py (the gate:
tests/test_contacts_cpu.py on the host build) as ONE set('qpos') + forward() of a batch whose environments are the poses,
then the published contact list -- ncon, contact_geom1 / 2, contact_dist / pos / frame, warning -- against the oracle's,
contact by contact and in order.  What only the device runs is what this reaches: the lane-parallel compaction and its
running base, the pair prefetch, trips past the first, which contacts survive a full cap, con_frame in global scratch,
the device-only accessors, the strided per-environment geom reads, the baked and the specialised kernels."""
import functools
import os

import numpy as np
import pytest

import contact_cases as cc
from dm_control_amd import mjcf_compiler as mc

pytestmark = pytest.mark.gpu

ALL_PAIRS = cc.PAIRS + cc.GUARDED
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dm_control_amd', 'suite', 'assets')
FIELDS = ('ncon', 'contact_geom1', 'contact_geom2', 'contact_dist', 'contact_pos', 'contact_frame', 'warning')


def _forward(model, qpos, precision, setup=None, **kw):
  """One set('qpos') + forward() of a fresh batch: ({field: (B, rows)}, info)."""
  from dm_control_amd.batch import BatchedPhysics
  b = BatchedPhysics(model, len(qpos), precision=precision, **kw)
  try:
    if setup is not None:
      setup(b)
    b.set('qpos', qpos)
    b.forward()
    b.sync()
    return {n: b.get(n) for n in FIELDS}, dict(b.info(), specialised=b.specialised)
  finally:
    b.close()


def _listings(f):
  return cc.listings(f.__getitem__, len(f['ncon']))


def _rows_past_ncon_are_blank(f, nconmax):
  """store_outputs: -1 in the geom rows, 0 in the real rows of every slot past ncon."""
  live = np.arange(nconmax)[None, :] < f['ncon']
  assert f['contact_geom1'].shape[1] == nconmax
  for n in ('contact_geom1', 'contact_geom2'):
    assert (f[n][~live] == -1).all() and (f[n][live] >= 0).all(), n
  for n, k in (('contact_dist', 1), ('contact_pos', 3), ('contact_frame', 9)):
    assert not f[n].reshape(len(live), nconmax, k)[~live].any(), n


def _report(what, prec, errs, left_out):
  print('MEASURED %s fp%d: dist %.3e pos %.3e normal %.3e frame %.3e, %.3f left out' %
        (what, prec, errs['dist'], errs['pos'], errs['normal'], errs['frame'], left_out))


# ---- single-pair scenes, generic kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', [64, 16])
@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('t1,t2', ALL_PAIRS, ids=['%s-%s' % p for p in ALL_PAIRS])
def test_pair_contacts_match_oracle(t1, t2, precision, lanes):
  case = cc.pair_case(t1, t2)
  f, info = _forward(case.model, case.qpos, precision, nconmax=8, lanes_per_env=lanes, specialise='off')
  assert info['lanes_per_env'] == lanes and info['static_id'] < 0, info
  _rows_past_ncon_are_blank(f, info['nconmax'])
  errs, left_out = cc.check_case(case, _listings(f), precision)
  _report(case.name, precision, errs, left_out)
  assert case.edge[:cc.NPOSE].mean() <= cc.EDGE_CAP      # (what fp32 leaves out of the sampled poses)
  cc.assert_within(errs, case.cls, precision, case.name)


def test_an_ellipsoid_against_a_box_is_refused_at_create_time():
  from dm_control_amd import _native
  from dm_control_amd.batch import BatchedPhysics
  with pytest.raises(_native.NativeError, match='not implemented'):
    BatchedPhysics(mc.compile_xml(cc.pair_xml(*cc.REFUSED)), 4, precision=32, specialise='off')


def test_parallel_capsules_keep_both_contacts_when_the_caller_asks_for_room():
  m = cc.pair_model('capsule', 'capsule')
  q = np.stack([p for n, _, _, p, _ in cc.directed_poses() if n.startswith('parallel capsules')])
  for precision in (64, 32):
    f, info = _forward(m, q, precision, nconmax=8, specialise='off')
    assert (info['nconmax'], info['njmax']) == (2, 8)
    assert (f['ncon'] == 2).all() and not f['warning'].any()
    f, info = _forward(m, q, precision, specialise='off')
    assert (info['nconmax'], info['njmax']) == (1, 4)      # the default caps count one contact per capsule-capsule pair
    assert (f['ncon'] == 1).all() and (f['warning'][:, cc.WARN_CONTACTFULL] == 1).all()


# ---- the heap: 75 candidate pairs, several trips of the pair loop, a full cap ----------------------------------------------------
@pytest.mark.parametrize('B', [5, 67])
@pytest.mark.parametrize('precision,lanes', [(64, 64), (64, 32), (64, 16), (32, 32)])
def test_heap_keeps_the_oracles_order_and_its_first_contacts_under_a_cap(precision, lanes, B):
  case = cc.heap_case(B)
  assert len(case.model.pair_geom1) == cc.HEAP_NPAIR > lanes      # (16 lanes: five trips)
  # (fp64 at 16 lanes: four environments share a wave, and their scratch fits the LDS only with fewer constraint rows
  # than 48 contacts can fill -- rows the contact list does not need: the host build lists the same contacts, CPU tier)
  njmax = 64 if (precision, lanes) == (64, 16) else 0
  for cap, nconmax in ((None, cc.HEAP_NCONMAX), (cc.HEAP_SMALL_CAP, cc.HEAP_SMALL_CAP)):
    f, info = _forward(case.model, case.qpos, precision, nconmax=nconmax, njmax=njmax, lanes_per_env=lanes, specialise='off')
    assert info['lanes_per_env'] == lanes and info['nconmax'] == nconmax, info
    _rows_past_ncon_are_blank(f, nconmax)
    errs, left_out = cc.check_case(case, _listings(f), precision, cap=cap)
    _report('heap cap %s' % cap, precision, errs, left_out)
    assert cap is None or (f['warning'][:, cc.WARN_CONTACTFULL] == 1).all()      # every state has more than the small cap
    cc.assert_within(errs, 'analytic', precision, 'heap')


@pytest.mark.parametrize('B', [5, 67])
def test_heap_contact_frames_in_lds_and_in_global_scratch_are_the_same_bits(B, monkeypatch):
  """60 dofs: by default con_frame lives in the environment's global scratch (offload level >= 2); DMC_JLEVEL=1 keeps it
  in LDS.  Only where the frames are stored differs: both lists match the oracle and each other to the bit."""
  case = cc.heap_case(B)
  out = {}
  for level in (None, '1'):
    monkeypatch.delenv('DMC_JLEVEL', raising=False)
    if level:
      monkeypatch.setenv('DMC_JLEVEL', level)
    f, info = _forward(case.model, case.qpos, 32, nconmax=cc.HEAP_NCONMAX, lanes_per_env=32, specialise='off')
    errs, _ = cc.check_case(case, _listings(f), 32)
    cc.assert_within(errs, 'analytic', 32, 'heap level %s' % level)
    out[level] = (f, info['global_scratch_bytes_per_env'])
  # the frames (9 reals per contact slot) are part of the default level's global scratch and not of level 1's
  assert out[None][1] - out['1'][1] >= 9*cc.HEAP_NCONMAX*4 and out['1'][1] > 0, (out[None][1], out['1'][1])
  for n in FIELDS:
    assert np.array_equal(out[None][0][n], out['1'][0][n]), n


def test_heap_in_a_specialised_kernel():
  """The one case that pays a compile (cached in-tree): the heap's own model-specialised fp32 kernel."""
  case = cc.heap_case(67)
  f, info = _forward(case.model, case.qpos, 32, nconmax=cc.HEAP_NCONMAX, specialise='build')
  assert info['specialised'] == 'attached' and info['static_id'] >= 1000, info
  errs, left_out = cc.check_case(case, _listings(f), 32)
  _report('heap specialised', 32, errs, left_out)
  cc.assert_within(errs, 'analytic', 32, 'heap specialised')


# ---- baked kernels at the production caps ---------------------------------------------------------------------------------------
def _asset(name):
  with open(os.path.join(ASSETS, name + '.xml')) as f:
    return mc.compile_xml(f.read())


def _cheetah_states(m, n):
  rs = np.random.RandomState(0)
  q = np.tile(m.qpos0, (n, 1))
  q[:, 1] -= rs.uniform(0.0, 0.35, n)      # rootz: the feet, the torso or the head into the floor
  q[:, 2] = rs.uniform(-1.2, 1.2, n)       # rooty
  q[:, 3:] += rs.uniform(-0.5, 0.5, (n, m.nq - 3))
  return q


def _humanoid_states(m, n):
  """The recipe of test_humanoid_forward_all_sensors_match_oracle (tests/test_gpu_suite.py)."""
  rs = np.random.RandomState(0)
  q = np.tile(m.qpos0, (n, 1))
  q[:, 2] = rs.uniform(0.05, 1.3, n)
  quat = rs.randn(n, 4)
  q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
  q[:, 7:] += rs.uniform(-0.4, 0.4, (n, m.nq - 7))
  return q


def _soccer_states(m, n):
  from dm_control_amd.composer.tasks import soccer
  rs = np.random.RandomState(0)
  q = np.tile(soccer.kickoff_qpos(m), (n, 1))
  bq = soccer.addresses(m)['ball_q']
  q[:, bq:bq + 3] = rs.uniform([-.6, -.6, .05], [.6, .6, .2], (n, 3))      # a scrum about the ball, everyone pressed into the pitch
  quat = rs.randn(n, 4)
  q[:, bq + 3:bq + 7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
  for x, y in soccer.addresses(m)['players']:      # root_x, root_y, root_z, steer, kick, roll
    q[:, x:x + 6] = rs.uniform([-.8, -.8, -.08, -3, -.3, -1], [.8, .8, 0, 3, .3, 1], (n, 6))
  return q


def _stacker_states(m, n):
  rs = np.random.RandomState(0)
  q = np.tile(m.qpos0, (n, 1))
  q[:, :8] = rs.uniform(-1.2, 1.2, (n, 8))      # the arm folded over the heap
  for k in range(4):                            # box k: x, z, y-rotation
    q[:, 8 + 3*k:11 + 3*k] = rs.uniform([-.35, .01, -1], [.35, .12, 1], (n, 3))
  return q


BAKED = {'cheetah': (_cheetah_states, 0), 'humanoid': (_humanoid_states, 24), 'soccer_2v2_boxhead': (_soccer_states, 24),
         'stacker': (_stacker_states, 48)}
NBAKED = 24


@functools.lru_cache(maxsize=None)
def baked_case(name):
  m = _asset(name)
  return cc.Case(name, m, BAKED[name][0](m, NBAKED), 'analytic')


@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('name', sorted(BAKED))
def test_baked_kernels_list_the_oracles_contacts_in_order(name, precision):
  case = baked_case(name)
  nconmax = BAKED[name][1]
  counts = np.array([r.ncon for r in case.refs])
  assert (counts > 0).sum() >= NBAKED//3 and counts.max() >= 6, counts      # contact-rich
  f, info = _forward(case.model, case.qpos, precision, nconmax=nconmax)
  if precision == 32 and name != 'stacker':      # (stacker has no baked kernel: the generic one, or its cached twin)
    assert 0 <= info['static_id'] < 1000, info
  print('%s fp%d: static_id %d, contacts %s' % (name, precision, info['static_id'], counts.tolist()))
  _rows_past_ncon_are_blank(f, info['nconmax'])
  errs, left_out = cc.check_case(case, _listings(f), precision, cap=info['nconmax'])
  _report(name, precision, errs, left_out)
  cc.assert_within(errs, 'analytic', precision, name)


# ---- per-environment geoms: the strided eg_data reads of narrow_phase ------------------------------------------------------------
def _env_geom_xml(t):
  return ('<mujoco><option gravity="0 0 0"/><worldbody>'
          '<geom name="fixed" type="box" size=".12 .09 .15" pos=".05 -.02 .1" quat=".9 .1 .3 .2" margin="%g"/>'
          '<body name="B" pos="0 0 1"><freejoint/><geom name="b" type="%s" size="%s" margin="%g"/></body>'
          '</worldbody></mujoco>') % (cc.MARGIN, t, cc.SIZES[t], cc.MARGIN)


@functools.lru_cache(maxsize=None)
def env_geom_case(t, n=33):
  """A free sphere / capsule about a world-fixed box whose size differs in every environment; the oracle of environment
  e has the size (and bounding radius) written into its own model."""
  m = mc.compile_xml(_env_geom_xml(t))
  g = m.name2id('fixed', 'geom')
  rs = np.random.RandomState(3)
  size = np.array(m.geom_size[g])[None]*rs.uniform(0.6, 1.4, (n, 3))
  q = np.zeros((n, 7))
  for e in range(n):
    d = rs.normal(size=3)
    q[e, :3] = np.array(m.geom_pos[g]) + d/np.linalg.norm(d)*rs.uniform(0.3, 0.9)*(np.linalg.norm(size[e]) + cc.RBOUND[t])
    q[e, 3:] = cc._quat(rs)      # pylint: disable=protected-access

  def edit(e):
    def apply(om):
      om.field('geom_size')[3*g:3*g + 3] = size[e]
      om.field('geom_rbound')[g] = np.linalg.norm(size[e])
    return apply
  return cc.Case('fixed box-%s' % t, m, q, 'analytic', move=slice(0, 3), edits=[edit(e) for e in range(n)]), size


@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('t', ['sphere', 'capsule'])
def test_per_environment_geom_sizes_reach_the_narrow_phase(t, precision):
  case, size = env_geom_case(t)
  counts = np.array([r.ncon for r in case.refs])
  assert (counts > 0).mean() >= 0.5
  # (the sizes matter: the oracle of the unedited model lists other contacts)
  assert any(cc.oracle_ref(case.model, q).pairs != r.pairs or
             not np.allclose(cc.oracle_ref(case.model, q).dist, r.dist, atol=1e-3) for q, r in zip(case.qpos, case.refs))

  def setup(b):
    b.set_env_geoms(['fixed'])
    b.set_env_geom('fixed', size=size)
  f, info = _forward(case.model, case.qpos, precision, setup=setup, nconmax=4, specialise='off')
  errs, left_out = cc.check_case(case, _listings(f), precision)
  _report(case.name, precision, errs, left_out)
  assert left_out <= 2/len(case.qpos)
  cc.assert_within(errs, 'analytic', precision, case.name)


# ---- the caps of the suite models ---------------------------------------------------------------------------------------------
def test_suite_assets_keep_their_caps_on_the_device():
  """info()['nconmax'] / ['njmax'] of every suite asset at its production cap: the parent commit's values."""
  from dm_control_amd.batch import BatchedPhysics
  for name, (asked, nconmax, njmax) in cc.SUITE_CAPS.items():
    b = BatchedPhysics(_asset(name), 2, precision=32, nconmax=asked)
    info = b.info()
    b.close()
    assert (info['nconmax'], info['njmax']) == (nconmax, njmax), (name, info)

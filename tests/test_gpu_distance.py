"""Batched geom distances on the GPU: one launch over the fixture's 32 states x 55 pairs (tests/golden/distance_cases.npz:
the fp64 twin's answers) in both precisions, the fp64 kernel against the host build of the same csrc/dist_core.h on the
device's own poses, a ragged launch with body members, live geom sizes, the stale-pose refusal, graph capture,
suite/proximity.wrap and mujoco_api.mj_geomDistance.  The bounds are the CPU tier's (tests/distance_cases.py)."""
import numpy as np
import pytest

import dist_emu_lib as emu
import dist_twin as tw
import distance_cases as dc
from dm_control_amd import mjcf_compiler as mc

pytestmark = pytest.mark.gpu

B = dc.NSTATE
NAMES = [g[0] for g in dc.GEOMS]
NAMED_PAIRS = [(NAMES[i], NAMES[j]) for i, j in dc.PAIRS]


def make_batch(model, precision, batch_size, **kw):
  from dm_control_amd.batch import BatchedPhysics
  return BatchedPhysics(model, batch_size, precision=precision, **kw)


def fixture_batch(precision, states=slice(0, B), model=None):
  """Environment e holds state e of the fixture, set with set('qpos') + forward()."""
  g = dc.load_golden()
  q = dc.qpos_of(g['pos'][states], g['quat'][states])
  b = make_batch(model if model is not None else mc.compile_xml(dc.xml(collide=False)), precision, len(q))
  b.set('qpos', q)
  b.forward()
  b.sync()
  return b, g


def device_geoms(b, e, sizes=None):
  """Twin-style geoms of environment e from the poses in device memory."""
  import torch
  torch.cuda.synchronize()
  m = b.model
  xp, xm = np.asarray(b.get('geom_xpos'), dtype=np.float64)[e].reshape(-1, 3), np.asarray(b.get('geom_xmat'), dtype=np.float64)[e].reshape(-1, 3, 3)
  size = np.asarray(m.geom_size if sizes is None else sizes, dtype=np.float64).reshape(-1, 3)
  return [tw.Geom(int(m.geom_type[i]), size[i], xp[i], xm[i]) for i in range(m.ngeom)]


def bounds(prec, ref):
  scale = np.maximum(1.0, np.abs(ref))
  exact = np.array([dc.exact_pair(p) for p in dc.PAIRS])
  return dc.F32_TOL*scale if prec == 32 else np.where(exact, dc.TOL_F64*scale, dc.TOLERANCE*scale + dc.E_TWIN)


@pytest.mark.parametrize('prec', [64, 32])
def test_fixture_batch_against_the_twin(prec):
  import torch
  from dm_control_amd import distance
  b, g = fixture_batch(prec)
  bd = distance.BatchDistance(b, NAMED_PAIRS, distmax=dc.DISTMAX)
  info = bd.info()
  assert (info['B'], info['npair'], info['block']) == (B, 55, 64) and info['lds_bytes'] <= 65536 and bd.skipped_geoms == []
  dist, fromto, normal, status = bd.query(fromto=True, normal=True, status='bits')
  assert tuple(dist.shape) == (B, 55) and tuple(fromto.shape) == (B, 55, 6) and status.dtype == torch.int32 and dist.device.type == 'cuda'
  assert torch.equal(bd.query(), dist)      # the outputs are independent of what else is asked for
  d, ft, n, st = (t.cpu().numpy().astype(np.float64) for t in (dist, fromto, normal, status))
  assert not (st.astype(np.int64) & 1).any() and 300 <= (st.astype(np.int64) >> 1).sum() <= 700      # every lane converged; EPA ran where cores overlap
  ref = np.minimum(g['dist'][:B], dc.DISTMAX)
  err = np.abs(d - ref)
  print('fp%d kernel worst |d - twin| / max(1, |d|): %.3e' % (prec, np.max(err/np.maximum(1.0, np.abs(ref)))))
  bound = bounds(prec, ref)
  assert np.all(err <= bound)
  near = d < dc.DISTMAX
  slack = bound + (1e-6 if prec == 32 else 0)
  assert near.all() and np.all(np.abs(np.linalg.norm(ft[..., 3:] - ft[..., :3], axis=-1) - np.abs(d)) <= slack)
  assert np.all(np.abs(np.linalg.norm(n, axis=-1) - 1) <= (1e-12 if prec == 64 else 1e-5))
  assert np.all(np.linalg.norm(ft[..., 3:] - ft[..., :3] - d[..., None]*n, axis=-1) <= slack)
  u = g['unique'][:B]
  werr = np.max(np.abs(ft - g['fromto'][:B]), axis=-1)
  print('fp%d kernel worst witness error where unique: %.3e' % (prec, werr[u].max()))
  assert u.mean() >= 1 - dc.UNIQUE_CAP and np.all(werr[u] <= dc.WITNESS_TOL[prec])


def test_fp64_kernel_equals_the_host_build_bit_for_bit():
  from dm_control_amd import distance
  b, _ = fixture_batch(64)
  bd = distance.BatchDistance(b, NAMED_PAIRS, distmax=dc.DISTMAX)
  dist, fromto, status = (t.cpu().numpy() for t in bd.query(fromto=True, status='bits'))
  differ = 0
  for e in range(B):
    G = device_geoms(b, e)
    r = emu.pairs(64, [G[p[0]] for p in dc.PAIRS], [G[p[1]] for p in dc.PAIRS], dc.DISTMAX, dc.TOLERANCE, dc.ITERATIONS)
    differ += int((r['dist'] != dist[e]).sum()) + int((r['fromto'] != fromto[e]).any(axis=-1).sum())
    assert np.array_equal(r['epa'], status[e] >> 1)
  print('fp64 kernel against the host build: %d of %d results differ in some bit' % (differ, 2*B*55))
  assert differ == 0


@pytest.mark.parametrize('prec', [64, 32])
def test_every_lane_of_a_wave_in_epa_runs_in_lds_passes(prec):
  """B = 128 (two full waves per pair) with pairs whose cores overlap in EVERY environment: all 64 lanes of a wave ask
  for a polytope, 21 (fp64) / 39 (fp32) fit at a time, so a wave runs four / two passes on shared slices.  The fp64 kernel
  must still equal the host build bit for bit, status included; fp32 stays within its bound of the fp64 host build."""
  from dm_control_amd import distance
  rs = np.random.RandomState(11)
  nb = 128
  pos = rs.uniform(-0.025, 0.025, (nb, dc.NBODY, 3)) + [0, 0, 0.5]      # centres within 0.05 of one another: inside every core
  quat = rs.normal(size=(nb, dc.NBODY, 4))
  quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
  b = make_batch(mc.compile_xml(dc.xml(collide=False)), prec, nb)
  b.set('qpos', dc.qpos_of(pos, quat))
  b.forward()
  b.sync()
  pairs = [('box0', 'box1'), ('sph0', 'box1'), ('cap0', 'box0'), ('ell0', 'box1'), ('cyl0', 'ell1')]
  ids = [(NAMES.index(a), NAMES.index(c)) for a, c in pairs]
  bd = distance.BatchDistance(b, pairs, distmax=dc.DISTMAX)
  assert 64 > 2*bd.info()['epa_lanes_per_pass'] or prec == 32
  dist, fromto, status = (t.cpu().numpy() for t in bd.query(fromto=True, status='bits'))
  assert np.all((status >> 1) == 1)      # every lane ran EPA
  worst = 0.0
  for e in range(nb):
    G = device_geoms(b, e)
    r = emu.pairs(64, [G[i] for i, _ in ids], [G[j] for _, j in ids], dc.DISTMAX, dc.TOLERANCE, dc.ITERATIONS)
    if prec == 64:
      assert np.array_equal(r['dist'], dist[e]) and np.array_equal(r['fromto'], fromto[e]) and np.array_equal(r['status'] != 0, (status[e] & 1) != 0), e
    else:
      err = np.abs(dist[e] - r['dist']) - r['gap']
      worst = max(worst, float(np.max(err/np.maximum(1.0, np.abs(r['dist'])))))
  if prec == 32:
    print('fp32 kernel, every lane in EPA: worst (|d - d_host64| - gap) / max(1, |d|): %.3e' % worst)
    assert worst <= dc.F32_TOL + dc.TOLERANCE


def body_model():
  return mc.compile_xml('<mujoco><option gravity="0 0 0"/><default><geom contype="0" conaffinity="0"/></default><worldbody><geom name="floor" type="plane" size="1 1 .1"/>'
                        '<body name="arm" pos="0 0 0.6"><freejoint/><geom name="u" type="capsule" size=".05 .2"/>'
                        '<geom name="f" type="box" size=".1 .08 .06" pos="0.05 0 .3"/></body>'
                        '<body name="ball" pos="0.4 0 0.5"><freejoint/><geom name="s" type="ellipsoid" size=".1 .07 .05"/></body></worldbody></mujoco>')


@pytest.mark.parametrize('prec', [64, 32])
def test_ragged_launch_body_members_and_distmax(prec):
  """B = 5, P = 3: fifteen lanes of one wave.  A body member is the minimum over its geoms; a pair beyond its own distmax
  reads distmax and zeros."""
  from dm_control_amd import distance
  m = body_model()
  rs = np.random.RandomState(3)
  q = np.tile(np.asarray(m.qpos0, dtype=np.float64), (5, 1))
  q[:, 7:10] = [0.1, 0.05, 0.75] + rs.uniform(-0.25, 0.25, (5, 3))
  q[:, 10:14] = rs.normal(size=(5, 4))
  q[:, 10:14] /= np.linalg.norm(q[:, 10:14], axis=1, keepdims=True)
  b = make_batch(m, prec, 5)
  b.set('qpos', q)
  b.forward()
  b.sync()
  bd = distance.BatchDistance(b, [(dict(body='arm'), 's'), ('s', dict(body='arm')), (dict(body='ball'), 'floor')], distmax=[5.0, 5.0, 0.6])
  each = distance.BatchDistance(b, [('u', 's'), ('f', 's'), ('s', 'floor')], distmax=5.0)
  d, ft, n, st = (t.cpu().numpy().astype(np.float64) for t in bd.query(fromto=True, normal=True, status=True))
  de, fe, ne = (t.cpu().numpy().astype(np.float64) for t in each.query(fromto=True, normal=True))
  assert not st.any() and len({tuple(x) for x in np.argmin(de[:, :2], axis=1)[:, None]}) == 2      # both geoms of the arm win somewhere
  tol = dc.TOLERANCE if prec == 64 else dc.F32_TOL
  for e in range(5):
    k = int(np.argmin(de[e, :2]))
    assert d[e, 0] == de[e, k] and np.array_equal(ft[e, 0], fe[e, k]) and np.array_equal(n[e, 0], ne[e, k])
    assert abs(d[e, 1] - d[e, 0]) <= tol      # the members swapped: from and to change places
    assert np.max(np.abs(ft[e, 1, :3] - ft[e, 0, 3:])) <= dc.WITNESS_TOL[prec] and np.max(np.abs(ft[e, 1, 3:] - ft[e, 0, :3])) <= dc.WITNESS_TOL[prec]
    G = device_geoms(b, e)
    ref = tw.distance(G[3], G[0])['dist']
    assert abs(de[e, 2] - ref) <= tol*max(1.0, abs(ref))
    if ref < 0.6:
      assert d[e, 2] == de[e, 2] and ft[e, 2].any()
    else:
      assert d[e, 2] == pytest.approx(0.6) and not ft[e, 2].any() and not n[e, 2].any()
  assert (de[:, 2] < 0.6).any() and (de[:, 2] >= 0.6).any()


def test_geom_sizes_are_read_live():
  from dm_control_amd import distance
  post = '<geom name="post" type="cylinder" size="0.1 0.3" pos="0.45 0.1 0.3" contype="0" conaffinity="0"/>'      # world-fixed: may differ per environment
  m = mc.compile_xml(dc.xml(collide=False, extra=post))
  b, g = fixture_batch(64, slice(0, 4), model=m)
  gid = lambda n: m.name2id(n, 'geom')
  pairs = [('sph0', 'box1'), ('post', 'ell1'), ('floor', 'cyl0')]
  ids = [(gid(a), gid(c)) for a, c in pairs]
  bd = distance.BatchDistance(b, pairs, distmax=dc.DISTMAX)
  d0 = bd.query().cpu().numpy()
  size = np.array(m.geom_size, dtype=np.float64)
  size[gid('box1')] *= 1.5
  b.set_model_real('geom_size', size)
  b.forward()
  b.sync()
  d1 = bd.query().cpu().numpy()
  assert np.all(d1[:, 0] < d0[:, 0]) and np.array_equal(d1[:, 1:], d0[:, 1:])
  b.set_env_geoms(['post'])
  b.set_env_geom('post', size=np.where(np.arange(4)[:, None] == 2, 0.5, 1.0)*size[gid('post')])
  b.forward()
  b.sync()
  d2 = bd.query().cpu().numpy()
  assert np.array_equal(d2[[0, 1, 3]], d1[[0, 1, 3]]) and d2[2, 0] == d1[2, 0] and d2[2, 2] == d1[2, 2] and d2[2, 1] > d1[2, 1]
  small = size.copy()
  small[gid('post')] *= 0.5
  for e, sz in ((1, size), (2, small)):
    G = device_geoms(b, e, sz)
    r = emu.pairs(64, [G[i] for i, _ in ids], [G[j] for _, j in ids], dc.DISTMAX)
    assert np.all(np.abs(r['dist'] - d2[e]) <= dc.TOL_F64)


def test_stale_poses_are_refused_and_a_graph_replays():
  import torch
  from dm_control_amd import _native, distance
  from dm_control_amd.batch import OUT, OUT_ALL
  m = mc.compile_xml(dc.xml(collide=False))
  fresh = make_batch(m, 32, 2)      # no launch yet: nothing to measure
  bd = distance.BatchDistance(fresh, NAMED_PAIRS[:3] + [('floor', 'floor')])      # (the default cutoff: infinity)
  with pytest.raises(_native.NativeError, match='output mask'):
    bd.query()
  fresh.forward()
  first = bd.query(fromto=True)
  assert bool(torch.isinf(first[0][:, 3]).all()) and not bool(first[1][:, 3].any()) and bool(torch.isfinite(first[0][:, :3]).all())      # plane-plane reads the cutoff
  b, g = fixture_batch(32, slice(0, 8))
  bd = distance.BatchDistance(b, NAMED_PAIRS, distmax=dc.DISTMAX)
  assert bd.output_mask == OUT['geom']
  b.set_output_mask(OUT_ALL & ~OUT['geom'])      # geom_xpos / geom_xmat masked out
  with pytest.raises(_native.NativeError, match='output mask'):
    bd.query()
  b.set_output_mask(OUT['xpos'] | OUT['xmat'])      # the mask the LAST LAUNCH ran with counts too
  b.step()
  b.set_output_mask(OUT_ALL)
  with pytest.raises(_native.NativeError, match='output mask'):
    bd.query()
  b.forward()
  plain = bd.query(fromto=True, normal=True, status=True)
  with pytest.raises(ValueError, match='out'):
    bd.query(out=[torch.zeros(3, device='cuda')])
  # a forward and a query recorded into one graph on one stream, replayed on another state
  out = [torch.zeros_like(t) for t in plain]
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    b.forward(stream=torch.cuda.current_stream().cuda_stream)
    bd.query(fromto=True, normal=True, status=True, out=out)
  b.set('qpos', dc.qpos_of(g['pos'][8:16], g['quat'][8:16]))
  for t in out:
    t.zero_()
  graph.replay()
  torch.cuda.synchronize()
  b.forward()
  eager = bd.query(fromto=True, normal=True, status=True)
  assert not torch.equal(eager[0], plain[0])      # the state did move
  for x, y in zip(out, eager):
    assert torch.equal(x, y)


def test_proximity_wrap_fused_cheetah():
  import torch
  from dm_control_amd import distance
  from dm_control_amd.suite import fused_env, proximity
  env = fused_env.make('cheetah', 'run', 64)
  m = env.model if hasattr(env, 'model') else env.physics.model
  names = m.names['geom']
  feet = [n for n in names if n in ('ffoot', 'bfoot', 'head')]
  assert len(feet) == 3
  ground = next(n for n in names if m.geom_type[names.index(n)] == 0)
  pairs = [(f, ground) for f in feet] + [(dict(body='torso'), ground), ('ffoot', 'bfoot')]
  penv = proximity.wrap(env, pairs, 1.0, proximity_only=True)
  obs = penv.reset()
  assert tuple(obs.shape) == (64, 5) and obs.dtype == env.dtype and obs.device.type == 'cuda'
  act = torch.zeros((64, m.nu), dtype=env.dtype, device=env.device)
  for _ in range(3):
    act.uniform_(-1, 1)
    obs, reward, done = penv.step(act)
  direct = distance.BatchDistance(penv.distance.batch, pairs, distmax=1.0).query()
  assert torch.equal(obs, direct) and torch.equal(obs, penv.read()) and reward.shape == (64,)
  assert bool((obs < 1.0).any()) and bool((obs[:, :3] > -0.2).all())
  b = penv.distance.batch
  for e in (0, 63):      # against the twin on the device's own poses
    G = device_geoms(b, e)
    for k, f in enumerate(feet):
      ref = min(tw.distance(G[names.index(f)], G[names.index(ground)])['dist'], 1.0)
      assert abs(float(obs[e, k]) - ref) <= dc.TOL_F32_ONE_STEP
  squashed = proximity.wrap(env, pairs, 1.0, scale='tanh')
  o2 = squashed.step(act)[0]
  assert set(o2) == {'state', 'proximity'} and torch.equal(o2['proximity'], torch.tanh(squashed.distance.query()/1.0))


def test_mj_geom_distance_on_a_hip_physics():
  from dm_control_amd import mujoco_api as mj
  g = dc.load_golden()
  model = mj.MjModel.from_xml_string(dc.xml(collide=False))
  data = mj.MjData(model)
  data.qpos[:] = dc.qpos_of(g['pos'][6], g['quat'][6])
  mj.mj_forward(model, data)
  checked = set()
  for pi in range(0, 55, 2):
    ft = np.zeros(6)
    d = mj.mj_geomDistance(model, data, dc.PAIRS[pi][0], dc.PAIRS[pi][1], dc.DISTMAX, ft)
    ref = g['dist'][6, pi]
    assert abs(d - ref) <= bounds(64, np.full(55, ref))[pi] + 1e-12
    if g['unique'][6, pi]:
      assert np.max(np.abs(ft - g['fromto'][6, pi])) <= dc.WITNESS_TOL[64]
    checked.add(d > 0)
  assert checked == {True, False}
  # sizes are the live ones, as the device unit reads them
  before = mj.mj_geomDistance(model, data, 1, 10, dc.DISTMAX, None)
  size = np.array(model._c.geom_size, dtype=np.float64)
  size[1] *= 0.5
  data._batch.set_model_real('geom_size', size)
  mj.mj_forward(model, data)
  after = mj.mj_geomDistance(model, data, 1, 10, dc.DISTMAX, None)
  assert after == pytest.approx(before + 0.5*dc.GEOMS[1][2][0], abs=1e-9)      # the sphere's radius halved

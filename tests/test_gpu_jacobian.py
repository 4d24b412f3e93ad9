"""Batched Jacobians on the GPU: the fixture model of tests/jacobian_cases.py in both precisions against the fp64 twin
evaluated on the device's own poses, the fp64 kernels against the host build of the same csrc/jac_core.h bit for bit, every
element written, ragged shapes, the CMU humanoid, determinism, graph capture and suite/effector.wrap.  The bounds are the
CPU tier's (tests/jacobian_cases.py)."""
import os

import numpy as np
import pytest

import jac_emu_lib as emu
import jacobian_cases as jc
from dm_control_amd import host_data
from dm_control_amd import mjcf_compiler as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 70      # one full wave plus a ragged tail
NV = 14 + 6 * jc.NBOX_GPU      # 62: the widest model a batch holds is nv = 64 (the CPU tier runs the header at nv = 74)


def make_batch(model, precision, batch_size, **kw):
  from dm_control_amd.batch import BatchedPhysics
  return BatchedPhysics(model, batch_size, precision=precision, **kw)


def fixture_batch(precision, batch_size=B, seed=jc.SEED):
  m = mc.compile_xml(jc.xml(jc.NBOX_GPU))
  qpos, qvel = jc.states(m, batch_size, seed)
  b = make_batch(m, precision, batch_size)
  b.set('qpos', qpos)
  b.set('qvel', qvel)
  b.forward()
  b.sync()
  return b


def device_state(b):
  """The state and the body poses in device memory, as fp64 numpy (B, ...)."""
  import torch
  torch.cuda.synchronize()
  g = lambda n: np.asarray(b.get(n), dtype=np.float64)
  return dict(qpos=g('qpos'), qvel=g('qvel'), xpos=g('xpos'), xquat=g('xquat'))


def wrench(n, T, seed=7):
  rs = np.random.RandomState(seed)
  return rs.uniform(-1, 1, (n, T, 3)), rs.uniform(-1, 1, (n, T, 3))


def check_against_twin(b, bj, targets, prec, joint_names=None, envs=None):
  import torch
  m, st = b.model, device_state(b)
  n, T = b.batch_size, len(targets)
  _, dev, dt = bj._torch()
  f, tq = wrench(n, T)
  pts = np.random.RandomState(3).uniform(-2, 2, (n, T, 3))
  jacp, jacr = bj.jac()
  jp_pt, jr_pt = bj.jac(point=torch.as_tensor(pts, dtype=dt, device=dev))
  vel, vel_local = bj.velocity(), bj.velocity(local=True)
  qfrc = bj.force(torch.as_tensor(f, dtype=dt, device=dev), torch.as_tensor(tq, dtype=dt, device=dev))
  C = len(bj.columns)
  assert tuple(jacp.shape) == tuple(jacr.shape) == (n, T, 3, C) and tuple(vel.shape) == (n, T, 6) and tuple(qfrc.shape) == (n, C)
  assert jacp.dtype == dt and jacp.device.type == 'cuda' and jacp.is_contiguous()
  got = {k: v.cpu().numpy().astype(np.float64) for k, v in dict(jacp=jacp, jacr=jacr, jp_pt=jp_pt, jr_pt=jr_pt, vel=vel, vel_local=vel_local,
                                                                 qfrc=qfrc).items()}
  # the inputs as the device holds them
  fq, tqq, ptq = (torch.as_tensor(a, dtype=dt).numpy().astype(np.float64) for a in (f, tq, pts))
  worst = {}
  for e in (range(n) if envs is None else envs):
    own = jc.twin(m, targets, st['qpos'][e], st['qvel'][e], st['xpos'][e], st['xquat'][e], joint_names=joint_names, force=fq[e], torque=tqq[e])
    loc = jc.twin(m, targets, st['qpos'][e], st['qvel'][e], st['xpos'][e], st['xquat'][e], joint_names=joint_names, point=ptq[e], local=True)
    for key, ref in (('jacp', own['jacp']), ('jacr', own['jacr']), ('vel', own['vel']), ('qfrc', own['qfrc']), ('jp_pt', loc['jacp']),
                     ('jr_pt', loc['jacr']), ('vel_local', loc['vel'])):
      err = np.abs(got[key][e] - ref).max()
      worst[key] = max(worst.get(key, 0.0), err / max(1.0, np.abs(ref).max()))
      assert err <= jc.bound(prec, ref), (e, key, err)
  print('fp%d kernels worst |x - twin| / max(1, |x|max): %s' % (prec, ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
  return got, st, (fq, tqq, ptq)


@pytest.mark.parametrize('prec', [64, 32])
def test_fixture_batch_against_the_twin(prec):
  from dm_control_amd import jacobian
  b = fixture_batch(prec)
  bj = jacobian.BatchJacobian(b, jc.TARGETS)
  info = bj.info()
  assert (info['B'], info['precision'], info['ntarget'], info['ncol'], info['block']) == (B, prec, 5, NV, 64)
  assert info['lds_bytes'] <= 65536 and info['force_lds_bytes'] <= 65536 and info['column_chunk'] < NV and info['max_chain_dofs'] == 14
  assert bj.output_mask == 0 and list(bj.columns) == list(range(NV))
  got, st, (f, tq, pts) = check_against_twin(b, bj, jc.TARGETS, prec)
  if prec == 64:      # the same header on the host, fed the device's own state: equal bits
    tb = jacobian.chain_tables(b.model, jc.TARGETS)
    differ = 0
    for e in range(B):
      r = emu.run(64, tb, st['qpos'][e], st['qvel'][e], force=f[e], torque=tq[e])
      rp = emu.run(64, tb, st['qpos'][e], st['qvel'][e], point=pts[e], local=True)
      for key, ref in (('jacp', r['jacp']), ('jacr', r['jacr']), ('vel', r['vel']), ('qfrc', r['qfrc']), ('jp_pt', rp['jacp']),
                       ('jr_pt', rp['jacr']), ('vel_local', rp['vel'])):
        differ += int((got[key][e] != ref).sum())
    print('fp64 kernels against the host build: %d results differ in some bit' % differ)
    assert differ == 0


@pytest.mark.parametrize('prec', [64, 32])
def test_every_element_is_written(prec):
  """out= tensors full of NaN, nv = 62: every target has whole column chunks off its chain (its dofs end at column 14; a
  chunk is 16 columns in fp64 and 32 in fp32).  No NaN may remain and the off-chain columns are exact zeros.  The issue
  asks for nv > 64 here; no batch can hold such a model (the step kernels stop at nv = 64), so the widest model that
  keeps the property is used, and tests/test_jacobian_cpu.py runs the same header at nv = 74."""
  import torch
  from dm_control_amd import jacobian
  b = fixture_batch(prec, 70)
  bj = jacobian.BatchJacobian(b, jc.MORE_TARGETS)
  _, dev, dt = bj._torch()
  n, T, C = bj.shape
  assert C == NV and C - 14 > bj.info()['column_chunk']
  nan = lambda *s: torch.full(s, float('nan'), dtype=dt, device=dev)
  jp, jr, jp1, vel, qf = nan(n, T, 3, C), nan(n, T, 3, C), nan(n, T, 3, C), nan(n, T, 6), nan(n, C)
  r = bj.jac(out=(jp, jr))
  assert r[0] is jp and r[1] is jr
  assert bj.jac(rot=False, out=jp1) is jp1
  bj.velocity(out=vel)
  bj.force(torch.ones(3, dtype=dt, device=dev), out=qf)
  for t in (jp, jr, jp1, vel, qf):
    assert not bool(torch.isnan(t).any())
  assert torch.equal(jp1, jp)
  for t, ch in enumerate(bj.tables['chains']):
    off = torch.as_tensor(np.setdiff1d(np.arange(C), ch['dof_id']), device=dev)
    assert off.numel() >= NV - 14
    assert not bool(jp[:, t][:, :, off].any()) and not bool(jr[:, t][:, :, off].any())
    on = torch.as_tensor(np.asarray(ch['dof_id']), device=dev)
    assert bool((jp[:, t][:, :, on].abs().amax(dim=(1, 2)) > 0).all())
  used = np.unique(np.concatenate([ch['dof_id'] for ch in bj.tables['chains']]))
  assert not bool(qf[:, torch.as_tensor(np.setdiff1d(np.arange(C), used), device=dev)].any())
  # a view that is not 16-byte aligned takes the scalar stores and still equals the aligned result
  flat = nan(n * T * 3 * C + 1)
  odd = flat[1:].view(n, T, 3, C)
  assert torch.equal(bj.jac(rot=False, out=odd), jp) and bool(torch.isnan(flat[0]))
  with pytest.raises(ValueError, match='out'):
    bj.jac(out=jp)
  with pytest.raises(ValueError, match='out'):
    bj.velocity(out=torch.zeros(3, device=dev))
  with pytest.raises(ValueError, match='point'):
    bj.jac(point=torch.zeros(n, T, 2, dtype=dt, device=dev))
  with pytest.raises(ValueError, match='dtype'):
    bj.force(torch.zeros(3, dtype=torch.float16, device=dev))
  with pytest.raises(ValueError, match='force'):
    bj.force(None)
  with pytest.raises(ValueError, match='shape'):
    bj.force(np.zeros((T + 1, 3)))


@pytest.mark.parametrize('prec', [64, 32])
def test_one_environment_one_target_ragged_columns(prec):
  from dm_control_amd import jacobian
  b = fixture_batch(prec, 1, seed=5)
  bj = jacobian.BatchJacobian(b, ['grasp'], joint_names=jc.SUBSET)
  C = len(bj.columns)
  assert bj.shape == (1, 1, 11) and C % bj.info()['column_chunk'] != 0 and C % 2 == 1
  check_against_twin(b, bj, ['grasp'], prec, joint_names=jc.SUBSET)
  # 37 columns: two chunks in fp32 and three in fp64, the last one ragged
  names = ['box%d_j' % k for k in (7, 0, 4, 2)] + ['root', 'h3', 'ball', 'slide', 'twist', 'h1']
  b2 = fixture_batch(prec, 3, seed=6)
  bj2 = jacobian.BatchJacobian(b2, jc.TARGETS[:2], joint_names=names)
  assert len(bj2.columns) == 37
  check_against_twin(b2, bj2, jc.TARGETS[:2], prec, joint_names=names)


@pytest.mark.parametrize('prec', [64, 32])
def test_cmu_humanoid_end_effectors(prec):
  from dm_control_amd import jacobian
  with open(os.path.join(ROOT, 'tests', 'golden', 'humanoid_CMU_V2019.xml')) as f:
    m = mc.compile_xml(f.read())
  n = 8
  rs = np.random.RandomState(12)
  qpos = np.tile(np.asarray(m.qpos0, dtype=np.float64), (n, 1)) + rs.uniform(-0.4, 0.4, (n, m.nq))
  for j in range(m.njnt):
    if int(m.jnt_type[j]) == 0:
      a = int(m.jnt_qposadr[j])
      q = rs.normal(size=(n, 4))
      qpos[:, a + 3:a + 7] = q / np.linalg.norm(q, axis=1, keepdims=True)
  b = make_batch(m, prec, n)
  b.set('qpos', qpos)
  b.set('qvel', rs.uniform(-1, 1, (n, m.nv)))
  b.forward()
  b.sync()
  targets = [dict(body=k) for k in ('lhand', 'rhand', 'lfoot', 'rfoot')]
  bj = jacobian.BatchJacobian(b, targets)
  info = bj.info()
  assert info['ncol'] == m.nv >= 56 and info['lds_bytes'] <= 65536 and info['column_chunk'] < info['ncol']
  got, st, _ = check_against_twin(b, bj, targets, prec)
  # mj_objectVelocity's own route: the device's cvel and subtree_com
  shapes = dict(xpos=(m.nbody, 3), xmat=(m.nbody, 3, 3), cvel=(m.nbody, 6), subtree_com=(m.nbody, 3))
  arr = {k: np.asarray(b.get(k), dtype=np.float64) for k in shapes}
  for e in range(n):
    get = lambda name, *shape: arr[name][e].reshape(shapes[name])
    for local, key in ((False, 'vel'), (True, 'vel_local')):
      ref = np.array([np.concatenate(host_data.object_velocity(m, 'xbody', m.name2id(t['body'], 'body'), get, local)) for t in targets])
      assert np.abs(got[key][e] - ref).max() <= jc.bound(prec, ref)


def test_determinism_and_independence_of_what_is_asked():
  import torch
  from dm_control_amd import jacobian
  b = fixture_batch(32, 130)
  bj = jacobian.BatchJacobian(b, jc.MORE_TARGETS)
  _, dev, dt = bj._torch()
  f, tq = (torch.as_tensor(a, dtype=dt, device=dev) for a in wrench(130, len(jc.MORE_TARGETS)))
  q1, q2 = bj.force(f, tq), bj.force(f, tq)
  assert torch.equal(q1, q2) and bool(q1.any())
  assert torch.equal(bj.force(f[0], tq[0]), bj.force(f[0].expand(130, -1, -1).contiguous(), tq[0].expand(130, -1, -1).contiguous()))
  assert torch.equal(bj.force(f[0, 0]), bj.force(f[0, 0].expand(130, len(jc.MORE_TARGETS), 3).contiguous()))
  jp, jr = bj.jac()
  assert torch.equal(bj.jac(rot=False), jp)
  bj.velocity()      # other launches in between change nothing
  bj.force(f)
  jp2, jr2 = bj.jac()
  assert torch.equal(jp2, jp) and torch.equal(jr2, jr)
  # numpy inputs and stream= behave as the tensors do
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    q3 = bj.force(f.cpu().numpy(), tq.cpu().numpy(), stream=s)
  s.synchronize()
  assert torch.equal(q3, q1)


def test_a_graph_of_the_three_launches_replays_after_a_step():
  import torch
  from dm_control_amd import jacobian
  b = fixture_batch(32, 40)
  bj = jacobian.BatchJacobian(b, jc.TARGETS, joint_names=['root', 'ball', 'slide', 'twist', 'h1', 'h2', 'h3'])
  _, dev, dt = bj._torch()
  n, T, C = bj.shape
  f = torch.as_tensor(wrench(n, T)[0], dtype=dt, device=dev)
  out = dict(jp=torch.zeros(n, T, 3, C, dtype=dt, device=dev), jr=torch.zeros(n, T, 3, C, dtype=dt, device=dev),
             vel=torch.zeros(n, T, 6, dtype=dt, device=dev), qf=torch.zeros(n, C, dtype=dt, device=dev))
  before = bj.jac()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    bj.jac(out=(out['jp'], out['jr']))
    bj.velocity(local=True, out=out['vel'])
    bj.force(f, out=out['qf'])
  for _ in range(3):
    b.step()
  b.sync()
  for t in out.values():
    t.zero_()
  graph.replay()
  torch.cuda.synchronize()
  jp, jr = bj.jac()
  assert not torch.equal(jp, before[0])      # the state did move
  assert torch.equal(out['jp'], jp) and torch.equal(out['jr'], jr)
  assert torch.equal(out['vel'], bj.velocity(local=True)) and torch.equal(out['qf'], bj.force(f))


def test_effector_wrap_fused_reacher():
  import torch
  from dm_control_amd import jacobian
  from dm_control_amd.suite import effector, fused_env
  env = fused_env.make('reacher', 'easy', 40)
  m = env.model if hasattr(env, 'model') else env.physics.model
  targets = [dict(body='finger'), dict(geom='finger'), dict(body='arm', com=True)]
  wenv = effector.wrap(env, targets, effector_only=True)
  obs = wenv.reset()
  assert tuple(obs.shape) == (40, 18) and obs.dtype == env.dtype and obs.device.type == 'cuda'
  direct = jacobian.BatchJacobian(wenv.jacobian.batch, targets)
  assert torch.equal(obs, direct.velocity().reshape(40, 18))      # after a reset
  act = torch.zeros((40, m.nu), dtype=env.dtype, device=env.device)
  for _ in range(3):
    act.uniform_(-1, 1)
    obs, reward, done = wenv.step(act)
  assert torch.equal(obs, direct.velocity().reshape(40, 18)) and torch.equal(obs, wenv.read()) and reward.shape == (40,)
  assert bool((obs.abs() > 0).any())
  # against the twin on the device's own state: the unit needed no pose array, the twin does -- a forward launch with every
  # output switched on writes the body poses at the qpos the step ended on
  from dm_control_amd.batch import OUT_ALL
  prec = int(direct.batch.precision)
  direct.batch.set_output_mask(OUT_ALL)
  direct.batch.forward()
  direct.batch.sync()
  st = device_state(direct.batch)
  for e in (0, 39):
    ref = jc.twin(m, targets, st['qpos'][e], st['qvel'][e], st['xpos'][e], st['xquat'][e])['vel']
    assert np.abs(obs[e].cpu().numpy().astype(np.float64).reshape(3, 6) - ref).max() <= jc.bound(prec, ref)
  both = effector.wrap(env, targets[:1], local=True)
  o2 = both.step(act)[0]
  assert set(o2) == {'state', 'effector_velocity'} and torch.equal(o2['effector_velocity'], both.jacobian.velocity(local=True).reshape(40, 6))

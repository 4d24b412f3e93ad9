"""Batched dynamics on the GPU: the fixture of tests/dynamics_cases.py in both precisions against the fp64 oracle evaluated on
the state the device holds, the fp64 kernels against the host build of the same csrc/dyn_core.h bit for bit, bias() against
the step kernel's own qfrc_bias, several environments per wave with a ragged last group, every element written, K = 1, 3,
7 and more than a chunk, determinism, independence of the lanes per environment, streams, graph capture and the
composition with BatchJacobian.  The bounds are the CPU tier's (tests/dynamics_cases.py)."""
import numpy as np
import pytest

import dyn_emu_lib as emu
import dynamics_cases as dc
import jacobian_cases as jc
from dm_control_amd import mjcf_compiler as mc

pytestmark = pytest.mark.gpu

B = 70      # one full wave of environments plus a ragged tail
NV = 62
_cache = {}


def make_batch(model, precision, batch_size, **kw):
  from dm_control_amd.batch import BatchedPhysics
  return BatchedPhysics(model, batch_size, precision=precision, **kw)


def batch_of(name, precision, batch_size=B):
  m = mc.compile_xml(dc.model_xml(name))
  qpos, qvel = dc.states(m, batch_size)
  b = make_batch(m, precision, batch_size)
  b.set('qpos', qpos)
  b.set('qvel', qvel)
  b.forward()
  b.sync()
  return b


def device_inputs(bd, n, nv, k=dc.K):
  """(qacc, vec) as device tensors and as the fp64 values the device holds."""
  import torch
  _, dev, dt = bd._torch()
  qacc, vec = dc.inputs(nv, n, k)
  tq, tv = torch.as_tensor(qacc, dtype=dt, device=dev), torch.as_tensor(vec, dtype=dt, device=dev)
  return tq, tv, tq.cpu().numpy().astype(np.float64), tv.cpu().numpy().astype(np.float64)


def world(name, prec):
  """The batch, its unit, the five results and the oracle's references on the device's own state, once per (model, precision)."""
  if (name, prec) not in _cache:
    import torch
    from dm_control_amd import dynamics
    b = batch_of(name, prec)
    bd = dynamics.BatchDynamics(b)
    nv = b.model.nv
    tq, tv, qacc, vec = device_inputs(bd, B, nv)
    res = dict(M=bd.mass_matrix(), bias=bd.bias(), inverse=bd.inverse(tq), mul=bd.mul(tv), solve=bd.solve(tv))
    torch.cuda.synchronize()
    g = lambda n: np.asarray(b.get(n), dtype=np.float64)
    st = dict(qpos=g('qpos'), qvel=g('qvel'), xpos=g('xpos'), xquat=g('xquat'), qfrc_bias=g('qfrc_bias'))
    ref = [dc.reference(b.model, st['qpos'][e], st['qvel'][e], qacc[e], vec[e]) for e in range(B)]
    _cache[(name, prec)] = dict(b=b, bd=bd, tq=tq, tv=tv, qacc=qacc, vec=vec, st=st, ref=ref, res=res,
                                got={k: v.cpu().numpy().astype(np.float64) for k, v in res.items()})
  return _cache[(name, prec)]


@pytest.mark.parametrize('prec', [64, 32])
def test_fixture_batch_against_the_references(prec):
  import torch
  w = world('fixture', prec)
  bd, got = w['bd'], w['got']
  info = bd.info()
  assert (info['B'], info['precision'], info['nv'], info['nbody']) == (B, prec, NV, 15)
  assert (info['lanes_per_env'], info['envs_per_block']) == (64, 1)      # nv = 62: the whole wave
  assert info['lds_bytes'] <= 65536 and info['rne_lds_bytes'] <= 65536 and info['chunk'] == 8
  assert bd.output_mask == 0
  _, dev, dt = bd._torch()
  for k, shape in (('M', (B, NV, NV)), ('bias', (B, NV)), ('inverse', (B, NV)), ('mul', (B, dc.K, NV)), ('solve', (B, dc.K, NV))):
    t = w['res'][k]
    assert tuple(t.shape) == shape and t.dtype == dt and t.device.type == 'cuda' and t.is_contiguous()
  worst = {}
  for e in range(B):
    ref = w['ref'][e]
    err = dc.check({k: got[k][e] for k in dc.OUTPUTS}, ref, w['vec'][e], prec, where=e)
    err['M_host'] = float(np.abs(got['M'][e] - ref['M_host']).max() / max(1.0, np.abs(ref['M_host']).max()))
    assert err['M_host'] <= dc.bound(prec, 'M')
    for k, v in err.items():
      worst[k] = max(worst.get(k, 0.0), v)
    assert np.array_equal(got['M'][e], got['M'][e].T)
  # inverse at the oracle's qacc_smooth against qfrc_smooth + qfrc_bias
  qs = np.stack([r['qacc_smooth'] for r in w['ref']])
  tqs = torch.as_tensor(qs, dtype=dt, device=dev)
  sm = bd.inverse(tqs).cpu().numpy().astype(np.float64)
  for e in range(B):
    r = w['ref'][e]
    held = tqs[e].cpu().numpy().astype(np.float64)      # (fp32: the acceleration the device holds)
    want = r['inverse_smooth'] + r['M'] @ (held - r['qacc_smooth'])
    err = float(np.abs(sm[e] - want).max() / max(1.0, np.abs(want).max()))
    worst['inverse_smooth'] = max(worst.get('inverse_smooth', 0.0), err)
    assert err <= dc.bound(prec, 'inverse_smooth'), (e, err)
  print('fp%d kernels, worst error / max(1, |ref|max): %s' % (prec, ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
  if prec == 64:      # the same header on the host, fed the device's own state: equal bits
    differ = 0
    for e in range(B):
      r = emu.run(64, bd.tables, w['st']['qpos'][e], w['st']['qvel'][e], w['qacc'][e], w['vec'][e])
      differ += sum(int((got[k][e] != r[k]).sum()) for k in dc.OUTPUTS)
    print('fp64 kernels against the host build: %d results differ in some bit' % differ)
    assert differ == 0


def test_fp64_bias_equals_the_step_kernels_qfrc_bias():
  """An independent device path: the forward launch's own mj_rne (csrc/step_core.h)."""
  w = world('fixture', 64)
  ref = w['st']['qfrc_bias']
  assert np.abs(ref).max() > 1
  assert np.abs(w['got']['bias'] - ref).max() <= dc.F64_TOL * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize('prec', [64, 32])
def test_cheetah_several_environments_per_wave_and_a_ragged_group(prec):
  w = world('cheetah', prec)
  info = w['bd'].info()
  assert (info['nv'], info['lanes_per_env'], info['envs_per_block']) == (9, 16, 4) and B % 4 != 0 and info['lds_bytes'] == 16384
  for e in range(B):
    dc.check({k: w['got'][k][e] for k in dc.OUTPUTS}, w['ref'][e], w['vec'][e], prec, where=e)
  if prec == 64:
    for e in (0, 1, 2, 3, 67, 68, 69):
      r = emu.run(64, w['bd'].tables, w['st']['qpos'][e], w['st']['qvel'][e], w['qacc'][e], w['vec'][e], lanes=16)
      assert all(np.array_equal(w['got'][k][e], r[k]) for k in dc.OUTPUTS)
    assert np.abs(w['got']['bias'] - w['st']['qfrc_bias']).max() <= dc.F64_TOL * max(1.0, np.abs(w['st']['qfrc_bias']).max())


@pytest.mark.parametrize('prec', [64, 32])
def test_every_element_is_written_and_k_right_hand_sides(prec):
  """out= tensors full of NaN come back without one; K = 1, 3, 7, more than one chunk (8), and the (B, nv) form; the
  environments' runs start on odd addresses (nv = 9: every other run of (B, nv) is off the 16-byte grid)."""
  import torch
  for name in ('cheetah', 'fixture'):
    w = world(name, prec)
    bd, nv = w['bd'], w['b'].model.nv
    _, dev, dt = bd._torch()
    nan = lambda *s: torch.full(s, float('nan'), dtype=dt, device=dev)
    M, bias, inv = nan(B, nv, nv), nan(B, nv), nan(B, nv)
    assert bd.mass_matrix(out=M) is M and bd.bias(out=bias) is bias and bd.inverse(w['tq'], out=inv) is inv
    assert torch.equal(M, w['res']['M']) and torch.equal(bias, w['res']['bias']) and torch.equal(inv, w['res']['inverse'])
    assert torch.equal(bd.inverse(w['tq'][0]), bd.inverse(w['tq'][0].expand(B, -1).contiguous()))      # the (nv,) form
    for K in (1, 3, 7, 11) if name == 'cheetah' else (1, 7, 9):
      _, tv, _, vec = device_inputs(bd, B, nv, K)
      mul, sol = nan(B, K, nv), nan(B, K, nv)
      bd.mul(tv, out=mul)
      bd.solve(tv, out=sol)
      gm, gs = mul.cpu().numpy().astype(np.float64), sol.cpu().numpy().astype(np.float64)
      assert np.isfinite(gm).all() and np.isfinite(gs).all()
      for e in (0, 1, 33, 68, 69):
        ref = w['ref'][e]
        dc.check(dict(mul=gm[e], solve=gs[e]), dict(M=ref['M'], mul=vec[e] @ ref['M'].T, solve=np.linalg.solve(ref['M'], vec[e].T).T),
                 vec[e], prec, where=(name, K, e))
      if K == 1:      # the (B, nv) form is the K = 1 form
        assert torch.equal(bd.mul(tv[:, 0].contiguous()), mul[:, 0]) and torch.equal(bd.solve(tv[:, 0].contiguous()), sol[:, 0])
        assert tuple(bd.solve(tv[:, 0].contiguous()).shape) == (B, nv)
    with pytest.raises(ValueError, match='out'):
      bd.bias(out=nan(B, nv + 1))
    with pytest.raises(ValueError, match='dtype'):
      bd.mul(torch.zeros(B, nv, dtype=torch.float64 if prec == 32 else torch.float32, device=dev))
    with pytest.raises(ValueError, match='K = 0'):
      bd.solve(torch.zeros(B, 0, nv, dtype=dt, device=dev))
    with pytest.raises(ValueError, match='shape'):
      bd.inverse(torch.zeros(B, nv + 1, dtype=dt, device=dev))


def test_two_launches_give_equal_bits_and_fp64_does_not_depend_on_the_lanes():
  import torch
  from dm_control_amd import dynamics
  for name, lanes in (('cheetah', (16, 32, 64)), ('humanoid', (32, 64))):
    w = world(name, 64)
    again = dict(M=w['bd'].mass_matrix(), bias=w['bd'].bias(), inverse=w['bd'].inverse(w['tq']), mul=w['bd'].mul(w['tv']), solve=w['bd'].solve(w['tv']))
    assert all(torch.equal(again[k], w['res'][k]) for k in dc.OUTPUTS)
    assert w['bd'].lanes_per_env == lanes[0]
    for l in lanes[1:]:
      other = dynamics.BatchDynamics(w['b'], lanes_per_env=l)
      assert other.info()['lanes_per_env'] == l
      res = dict(M=other.mass_matrix(), bias=other.bias(), inverse=other.inverse(w['tq']), mul=other.mul(w['tv']), solve=other.solve(w['tv']))
      assert all(torch.equal(res[k], w['res'][k]) for k in dc.OUTPUTS), (name, l)
  for e in (0, 69):      # humanoid: the bounds too
    w = world('humanoid', 64)
    dc.check({k: w['got'][k][e] for k in dc.OUTPUTS}, w['ref'][e], w['vec'][e], 64, where=e)
  with pytest.raises(ValueError, match='too small for the model'):
    dynamics.BatchDynamics(world('fixture', 64)['b'], lanes_per_env=16)
  w32 = world('fixture', 32)
  assert torch.equal(w32['bd'].solve(w32['tv']), w32['res']['solve']) and torch.equal(w32['bd'].bias(), w32['res']['bias'])


def test_a_non_default_stream_and_a_graph_of_solve_and_bias():
  import torch
  w = world('fixture', 32)
  bd, b = w['bd'], w['b']
  _, dev, dt = bd._torch()
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    x = bd.solve(w['tv'], stream=s)
    c = bd.bias(stream=s)
  s.synchronize()
  assert torch.equal(x, w['res']['solve']) and torch.equal(c, w['res']['bias'])
  # one capture of solve + bias on a single stream, after the warm-up calls above
  out = dict(x=torch.zeros(B, dc.K, NV, dtype=dt, device=dev), c=torch.zeros(B, NV, dtype=dt, device=dev))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    bd.solve(w['tv'], out=out['x'])
    bd.bias(out=out['c'])
  for t in out.values():
    t.zero_()
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(out['x'], w['res']['solve']) and torch.equal(out['c'], w['res']['bias'])


@pytest.mark.parametrize('prec', [64, 32])
def test_operational_space_inertia_with_the_jacobian_unit(prec):
  """J solve(J') for the hand's translational Jacobian (K = 3): symmetric positive definite, and J M^-1 J' of numpy on
  the references (the twin's Jacobian on the device's poses, the oracle's qM).  fp64: the project's 1e-9.  fp32: the
  bound of a solve carried forward -- its backward-error bound times cond(M) -- plus the Jacobian's own fp32 bound on
  both factors, relative to max(1, |reference|max)."""
  import torch
  from dm_control_amd import jacobian
  w = world('fixture', prec)
  bj = jacobian.BatchJacobian(w['b'], ['grasp'])
  J = bj.jac(rot=False)[:, 0].contiguous()      # (B, 3, nv)
  X = w['bd'].solve(J)                          # (B, 3, nv) = (M^-1 J')'
  lam = torch.matmul(J, X.transpose(1, 2)).cpu().numpy().astype(np.float64)
  for e in range(B):
    ref = w['ref'][e]
    Jr = jc.twin(w['b'].model, ['grasp'], w['st']['qpos'][e], w['st']['qvel'][e], ref['xpos'], ref['xquat'])['jacp'][0]
    want = Jr @ np.linalg.solve(ref['M'], Jr.T)
    scale = max(1.0, np.abs(want).max())
    tol = dc.F64_TOL if prec == 64 else dc.F32_TOL['solve'] * np.linalg.cond(ref['M']) + 2 * jc.F32_TOL
    assert np.abs(lam[e] - want).max() <= tol * scale, (e, np.abs(lam[e] - want).max(), tol * scale)
    assert np.abs(lam[e] - lam[e].T).max() <= tol * scale
    assert np.all(np.linalg.eigvalsh(0.5 * (lam[e] + lam[e].T)) > 0)

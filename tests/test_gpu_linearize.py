"""Batched linearisation on the GPU: the leg of tests/linearize_cases.py (B = 5: 265 scratch environments, several waves and a
ragged tail) with the fp64 kernels against the host build of the same csrc/lin_core.h bit for bit and against the numpy
twin evaluated on the state the device holds; cheetah and humanoid; an fp32 batch on an fp64 and on an fp32 scratch batch;
chunking, clamped controls, the untouched source batch, output hygiene, repeatability, streams, nstep, forward differences,
RK4 and the warning mask.  The bounds are tests/linearize_cases.py's (measured values beside them)."""
import numpy as np
import pytest

import lin_emu_lib as emu
import lin_twin as tw
import linearize_cases as lc

pytestmark = pytest.mark.gpu

STATE = ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart', 'qfrc_applied', 'time')
STEPPED = ('qpos', 'qvel', 'act', 'sensordata')
_cache = {}


def make_batch(name, precision, envs=None, **kw):
  """A batch of model `name` holding the states of `envs` ((state index, control) pairs; default: linearize_cases.ENVS)."""
  from dm_control_amd.batch import BatchedPhysics
  m = lc.model(name)
  st = lc.env_states(name, envs)
  b = BatchedPhysics(m, len(st), precision=precision, **kw)
  for k in STATE:
    if np.size(st[0][k]):
      b.set(k, np.stack([np.ravel(s[k]) for s in st]))
  b.sync()
  return b


def held(b):
  """The state the device holds, per environment, as fp64."""
  g = {k: np.asarray(b.get(k), dtype=np.float64) for k in STATE}
  return [{k: g[k][e].copy() for k in STATE} for e in range(b.batch_size)]


def numpy_of(tensors):
  return [t.cpu().numpy().astype(np.float64) for t in tensors]


def world(name, prec=64, scratch=64, eps=lc.EPS, centered=True, nstep=1):
  """The batch, its unit, A .. D and the twin's references on the device's own state, once per configuration."""
  key = (name, prec, scratch, eps, centered, nstep)
  if key not in _cache:
    import torch
    from dm_control_amd import linearize
    b = make_batch(name, prec)
    lin = linearize.BatchLinearization(b, eps=eps, centered=centered, nstep=nstep, precision=scratch)
    res = lin.transition(sensors=True)
    torch.cuda.synchronize()
    st = held(b)
    ref = [tw.transition_fd(b.model, s, eps, centered, nstep) for s in st]
    _cache[key] = dict(b=b, lin=lin, res=res, got=numpy_of(res), st=st, ref=ref)
  return _cache[key]


def judge(key, got, refs, store_ulps=0.0):
  """The worst error of A .. D (`got`: four (B, ...) arrays) against the twin's `refs`, separately over the contact-free
  environments and those in contact, printed and held against tests/linearize_cases.py's bound for `key`.  store_ulps:
  fp32 outputs -- the rounding of the store, relative to each matrix's own largest entry, comes on top."""
  worst = dict(free=0.0, contact=0.0)
  for e, ref in enumerate(refs):
    kind = 'contact' if ref['ncon'].max() > 0 else 'free'
    for g, k in zip(got, 'ABCD'):
      r = ref[k]
      if r.size:
        slack = store_ulps * np.finfo(np.float32).eps * np.abs(r).max() / max(1.0, np.abs(r).max())
        worst[kind] = max(worst[kind], lc.rel_err(g[e], r) - slack)
  for kind, err in worst.items():
    bound = lc.device_bound(key, kind)
    print('MEASURED %s, %s environments: worst error of A .. D against the twin / max(1, |ref|max) = %.3g (bound %.3g)' % (key, kind, err, bound))
    assert err <= bound, (key, kind, err, bound)


def check(w, key, store_ulps=0.0):
  judge(key, w['got'], w['ref'], store_ulps)


def test_leg_fp64_equals_the_host_build_and_meets_the_twin():
  import torch
  w = world('leg')
  b, lin, m = w['b'], w['lin'], w['b'].model
  info = lin.info()
  assert (info['B'], info['columns'], info['nx'], info['nu'], info['nsensordata']) == (5, 53, 23, 3, 8)
  assert (info['scratch_envs'], info['chunk'], info['chunks'], info['precision'], info['scratch_precision']) == (265, 5, 1, 64, 64)
  assert lin.scratch.legacy_step is False
  A, Bm, C, D = w['res']
  for t, shape in ((A, (5, 23, 23)), (Bm, (5, 23, 3)), (C, (5, 8, 23)), (D, (5, 8, 3))):
    assert tuple(t.shape) == shape and t.dtype == torch.float64 and t.device.type == 'cuda' and t.is_contiguous()
  # the stepped columns, read back, through the host build of the difference: equal bits
  sc = {k: np.asarray(lin.scratch.get(k), dtype=np.float64) for k in STEPPED}
  P = 53
  differ = 0
  for e in range(5):
    _, flags = emu.fan(64, m, lin.tables, lc.EPS, w['st'][e])
    want = emu.diff(64, m, lin.tables, lc.EPS, {k: sc[k][e * P:(e + 1) * P] for k in STEPPED}, flags)
    differ += sum(int((g[e] != x).sum()) for g, x in zip(w['got'], want))
  print('fp64 difference kernel against the host build: %d results differ in some bit' % differ)
  assert differ == 0
  assert (lin.warnings().cpu().numpy() == 0).all()
  # the fan-out alone: the scratch batch's state equals the host build's columns bit for bit
  assert lin.fan_out() == 5
  torch.cuda.synchronize()
  fields = ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart', 'qfrc_applied', 'time')
  sc = {k: np.asarray(lin.scratch.get(k), dtype=np.float64) for k in fields}
  assert not np.asarray(lin.scratch.get('warning')).any()
  differ = 0
  for e in range(5):
    cols, _ = emu.fan(64, m, lin.tables, lc.EPS, w['st'][e])
    differ += sum(int((sc[k][e * P:(e + 1) * P] != cols[k]).sum()) for k in fields)
  print('fp64 fan-out kernel against the host build: %d values differ in some bit' % differ)
  assert differ == 0
  # end to end against the twin on the state the device holds
  check(w, 'leg')
  # the clamped controls of the last environment: one-sided columns as in the twin, and B and D say so
  assert tuple(w['ref'][4]['flags']) == (tw.BACK, tw.FWD | tw.BACK, tw.FWD)


@pytest.mark.parametrize('name', ['cheetah', 'humanoid'])
def test_suite_models_fp64_against_the_twin(name):
  w = world(name)
  assert w['lin'].info()['columns'] == dict(cheetah=49, humanoid=151)[name]
  check(w, name)


def test_fp32_batch_on_an_fp64_scratch_batch():
  import torch
  w = world('leg', prec=32, scratch=64)
  assert all(t.dtype == torch.float32 for t in w['res'])
  assert (w['lin'].info()['precision'], w['lin'].info()['scratch_precision']) == (32, 64)
  # the twin runs at the fp32 state the device holds; the outputs are fp32 tensors: half an ulp of the store on top
  check(w, 'leg', store_ulps=0.5)


@pytest.mark.parametrize('name', ['leg', 'cheetah'])
def test_fp32_batch_on_an_fp32_scratch_batch(name):
  """precision=32 at eps = 2**-10 against the fp64 twin at the same eps: 4 x what the CPU tier's fp32 host pipeline gives."""
  w = world(name, prec=32, scratch=32, eps=lc.EPS32)
  worst = max(lc.worst([g[e] for g in w['got']], ref) for e, ref in enumerate(w['ref']))
  bound = 4 * lc.PIPELINE_F32_MEASURED[name]
  print('MEASURED %s fp32 scratch: worst error against the fp64 twin / max(1, |ref|max) = %.3g (bound %.3g)' % (name, worst, bound))
  assert worst <= bound, (name, worst, bound)


def test_chunks_give_the_bits_of_one_pass():
  import torch
  from dm_control_amd import linearize
  w = world('leg')
  lin = linearize.BatchLinearization(w['b'], max_scratch_envs=2 * 53 + 10)
  info = lin.info()
  assert (info['chunk'], info['chunks'], info['scratch_envs']) == (2, 3, 106)      # chunks of 2, 2 and 1
  res = lin.transition(sensors=True)
  torch.cuda.synchronize()
  for a, b in zip(res, w['res']):
    assert torch.equal(a, b)
  assert (lin.warnings().cpu().numpy() == 0).all()
  with pytest.raises(ValueError, match='needs 53 scratch environments'):
    linearize.BatchLinearization(w['b'], max_scratch_envs=52)
  with pytest.raises(ValueError, match='fp64 batch'):
    linearize.BatchLinearization(w['b'], precision=32)


def test_controls_at_both_limits():
  import torch
  from dm_control_amd import linearize
  ctrls = [(1.0, 0.3, -0.05), (-1.0, -2.0, 0.05), (1.5, 0.0, 0.0)]      # upper / lower, lower / upper, outside / inside
  flags = [(tw.BACK, 3, tw.FWD), (tw.FWD, 3, tw.BACK), (0, 3, 3)]
  for centered in (True, False):
    b = make_batch('leg', 64, [(1, c) for c in ctrls])
    lin = linearize.BatchLinearization(b, centered=centered)
    got = numpy_of(lin.transition(sensors=True))
    torch.cuda.synchronize()
    refs = []
    for e, s in enumerate(held(b)):
      ref = tw.transition_fd(b.model, s, lc.EPS, centered)
      refs.append(ref)
      want = tuple(f if centered or f != 3 else tw.FWD for f in flags[e])
      assert tuple(ref['flags']) == want
      for k, f in enumerate(want):
        if f == 0:      # no valid nudge: an exact zero column
          assert not got[1][e][:, k].any() and not got[3][e][:, k].any() and not ref['B'][:, k].any()
        else:
          assert got[1][e][:, k].any()
    judge('leg_limits' if centered else 'leg_limits_forward', got, refs)
    lin.close()
    b.close()


def test_source_batch_is_unchanged_and_outputs_are_fully_written():
  import torch
  from dm_control_amd import linearize
  b = make_batch('leg', 64)
  names = ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart', 'time')
  before = {k: np.asarray(b.get(k)).copy() for k in names}
  lin = linearize.BatchLinearization(b)
  _, dev, dt = lin._torch()
  out = tuple(torch.full(s, float('nan'), dtype=dt, device=dev) for s in ((5, 23, 23), (5, 23, 3), (5, 8, 23), (5, 8, 3)))
  res = lin.transition(sensors=True, out=out)
  torch.cuda.synchronize()
  assert all(r is o for r, o in zip(res, out)) and not any(torch.isnan(o).any().item() for o in out)
  ab = lin.transition(out=tuple(torch.full_like(o, float('nan')) for o in out[:2]))
  assert len(ab) == 2 and torch.equal(ab[0], out[0]) and torch.equal(ab[1], out[1])      # the same A, B without the sensors
  for k in names:
    assert np.asarray(b.get(k)).tobytes() == before[k].tobytes(), k
  w = world('leg')
  for a, r in zip(out, w['res']):
    assert torch.equal(a, r)      # another batch holding the same state, another object: the same bits
  with pytest.raises(ValueError, match='out'):
    lin.transition(out=(out[0],))
  with pytest.raises(ValueError, match='out'):
    lin.transition(out=(out[0], out[1].float()))


def test_repeatable_and_stream_ordered():
  import torch
  w = world('leg')
  lin = w['lin']
  again = lin.transition(sensors=True)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    third = lin.transition(sensors=True)
  raw = lin.transition(sensors=True, stream=side)
  side.synchronize()
  torch.cuda.synchronize()
  for a, b, c, d in zip(w['res'], again, third, raw):
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


@pytest.mark.parametrize('key,kw', [('leg_nstep3', dict(nstep=3)), ('leg_forward', dict(centered=False))])
def test_modes_against_the_twin(key, kw):
  w = world('leg', **kw)
  assert w['lin'].info()['columns'] == (53 if kw.get('centered', True) else 30)
  check(w, key)


def test_rk4_model_against_the_twin():
  w = world('acrobot')
  assert int(w['b'].model.opt.integrator) == 1 and w['lin'].info()['columns'] == 11 and w['lin'].info()['nsensordata'] == 0
  assert tuple(w['res'][2].shape) == (2, 0, 4) and tuple(w['res'][3].shape) == (2, 0, 1)
  check(w, 'acrobot')


def test_warnings_name_the_environment_that_ran_out_of_contacts():
  import torch
  from dm_control_amd import linearize
  b = make_batch('leg', 64, [(0, None), (3, None), (1, None)])      # 0, 4 and 1 contacts
  lin = linearize.BatchLinearization(b, nconmax=1)
  assert lin.scratch.info()['nconmax'] == 1
  lin.transition()
  warn = lin.warnings().cpu().numpy()
  torch.cuda.synchronize()
  full = 1 << 1      # mjWARN_CONTACTFULL
  assert warn.dtype == np.int32 and warn.shape == (3,)
  assert warn[0] == 0 and warn[2] == 0 and warn[1] & full, warn
  ok = linearize.BatchLinearization(b)
  ok.transition()
  assert (ok.warnings().cpu().numpy() == 0).all()

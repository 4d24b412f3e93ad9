"""dm_control_amd.host_data: the derivations and the state layout that `physics.Physics` and `mujoco_api.MjData` share,
on the fp64 oracle stand-in -- batched calls against single ones, both facades against each other and against the oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dm_control_amd import host_data  # noqa: E402
from dm_control_amd import mjcf_compiler as mc  # noqa: E402
from dm_control_amd import mujoco_api as mj  # noqa: E402
from dm_control_amd import physics as physics_lib  # noqa: E402
from dm_control_amd.suite import common  # noqa: E402
from joint_frames_walk import joint_frames_walk  # noqa: E402
from test_facade_cpu import _TENDON_XML  # noqa: E402
from test_facade_dropin import ARM, _random_state  # noqa: E402
from test_mujoco_api import _BALL_CHAIN, _shake  # noqa: E402


@pytest.fixture
def both_facades(oracle_backend, monkeypatch):
  monkeypatch.setattr(mj, 'BatchedPhysics', oracle_backend.OracleBatch)
  return oracle_backend


@pytest.mark.parametrize('name', ['ARM', 'humanoid_CMU.xml'])
def test_joint_frames_batched_equals_single_equals_the_oracle(name):
  from oracle.oracle import OraclePhysics
  m = mc.compile_xml(ARM if name == 'ARM' else common.read_model(name))
  o = OraclePhysics(m)
  states = []
  for seed in range(3):
    o.qpos[:] = _random_state(m, seed)
    o.forward()
    states.append([np.array(a, dtype=np.float64) for a in (
        o.qpos, o.xpos.reshape(-1, 3), o.xquat.reshape(-1, 4), o.field('mocap_pos'), o.field('mocap_quat'),
        o.xanchor.reshape(-1, 3), o.xaxis.reshape(-1, 3))])
  qpos, xpos, xquat, mpos, mquat, want_anchor, want_axis = (np.stack(a) for a in zip(*states))
  anchor, axis = host_data.joint_frames(m, qpos, xpos, xquat)      # B = 3 in one call
  assert anchor.shape == axis.shape == (3, m.njnt, 3)
  for e in range(3):
    one = host_data.joint_frames(m, qpos[e], xpos[e], xquat[e])
    np.testing.assert_array_equal(anchor[e], one[0])
    np.testing.assert_array_equal(axis[e], one[1])
  walk = joint_frames_walk(m, qpos, xpos, xquat, mpos, mquat)
  for got, ref in ((anchor, want_anchor), (axis, want_axis), (anchor, walk[0]), (axis, walk[1])):
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-14)


def test_tendon_arrays_through_both_facades(both_facades):
  """MjData's ten_length / ten_velocity / wrap_xpos against the oracle (as tests/test_facade_cpu.py checks the Physics
  facade's), and a Physics batch holding two different states against the per-environment values."""
  from oracle.oracle import OracleModel, OraclePhysics
  m = mj.MjModel.from_xml_string(_TENDON_XML)
  d = mj.MjData(m)
  c = m._c
  d.qpos[:] = [0.3, -0.5, 0.1]
  d.qvel[:] = [1.0, -2.0, 0.5]
  mj.mj_forward(m, d)
  o = OraclePhysics(OracleModel(c))
  states, served = [], []
  for _ in range(4):
    o.qpos[:], o.qvel[:] = d.qpos, d.qvel
    o.forward()
    np.testing.assert_allclose(d.ten_length, np.asarray(o.ten_length), rtol=0, atol=1e-12)
    J = np.asarray(o.ten_J).reshape(c.ntendon, c.nv)
    np.testing.assert_allclose(d.ten_velocity, J @ np.asarray(o.qvel), rtol=0, atol=1e-12)
    # wrap_xpos: the two end points of every segment of a spatial tendon, zero rows elsewhere (fixed tendons, last sites)
    want = np.zeros((c.nwrap, 6))
    for t in host_data.spatial_tendons(c):
      for w in range(int(c.tendon_adr[t]), int(c.tendon_adr[t] + c.tendon_num[t]) - 1):
        want[w] = np.r_[d.site_xpos[c.wrap_objid[w]], d.site_xpos[c.wrap_objid[w + 1]]]
    assert len(host_data.spatial_tendons(c)) == 2 and np.abs(want).sum(axis=1).astype(bool).sum() == 3
    np.testing.assert_array_equal(d.wrap_xpos, want)
    states.append((d.qpos.copy(), d.qvel.copy()))
    served.append((d.ten_length.copy(), d.ten_velocity.copy()))
    mj.mj_step(m, d, 25)
    mj.mj_forward(m, d)
  assert abs(served[-1][1]).max() > 0.1
  single = physics_lib.Physics.from_xml_string(_TENDON_XML)
  pair = physics_lib.Physics.from_xml_string(_TENDON_XML, batch_size=2)
  for k in (0, 2):
    per_env = []
    for qpos, qvel in states[k:k + 2]:
      with single.reset_context():
        single.data.qpos, single.data.qvel = qpos, qvel
      per_env.append((np.array(single.data.ten_length), np.array(single.data.ten_velocity)))
    with pair.reset_context():
      pair.data.qpos = np.stack([s[0] for s in states[k:k + 2]])
      pair.data.qvel = np.stack([s[1] for s in states[k:k + 2]])
    for e in range(2):
      np.testing.assert_array_equal(pair.data.ten_length[e], per_env[e][0])
      np.testing.assert_array_equal(pair.data.ten_velocity[e], per_env[e][1])
      np.testing.assert_array_equal(per_env[e][0], served[k + e][0])      # one function: MjData served the same numbers
      np.testing.assert_array_equal(per_env[e][1], served[k + e][1])
  single.free()
  pair.free()


def test_object_velocity_is_one_function_behind_both_facades(both_facades):
  m = mj.MjModel.from_xml_string(_BALL_CHAIN)
  d = mj.MjData(m)
  _shake(m, d)
  p = physics_lib.Physics(m._c)
  with p.reset_context():
    p.data.qpos, p.data.qvel, p.data.act, p.data.ctrl = d.qpos, d.qvel, d.act, d.ctrl
  np.testing.assert_array_equal(p.data.cvel, d.cvel)
  ids = {'body': ('fore', mj.mjtObj.mjOBJ_BODY), 'xbody': ('fore', mj.mjtObj.mjOBJ_XBODY),
         'geom': (3, mj.mjtObj.mjOBJ_GEOM), 'site': ('tip', mj.mjtObj.mjOBJ_SITE)}
  for kind, (obj, objtype) in ids.items():
    objid = obj if isinstance(obj, int) else mj.mj_name2id(m, int(objtype), obj)
    for local in (False, True):
      res = np.zeros(6)
      mj.mj_objectVelocity(m, d, int(objtype), objid, res, int(local))
      assert np.abs(res).min() > 0
      for key in (kind, int(objtype)):      # by name and by mjtObj
        v = p.data.object_velocity(obj, key, local_frame=local)
        np.testing.assert_array_equal(v[1], res[:3])      # (linear, angular) there, (angular, linear) here
        np.testing.assert_array_equal(v[0], res[3:])
  with pytest.raises(ValueError):
    p.data.object_velocity(0, 'joint')
  with pytest.raises(mj.FatalError):
    mj.mj_objectVelocity(m, d, int(mj.mjtObj.mjOBJ_JOINT), 0, np.zeros(6), 0)
  p.free()


def test_state_layout_is_one_table_behind_both_facades(both_facades):
  m = mj.MjModel.from_xml_string(ARM)      # (a mocap body: mocap_pos / mocap_quat have a size)
  p = physics_lib.Physics(m._c)
  c = m._c
  bits = [1 << k for k in range(13)]
  assert int(mj.mjtState.mjNSTATE) == host_data.NSTATE == 13
  sizes = dict(zip(bits, (1, c.nq, c.nv, c.na, c.nv, c.nu, c.nv, 6 * c.nbody, c.neq, 3 * c.nmocap, 4 * c.nmocap, 0, 0)))
  for sig in bits + [int(mj.mjtState.mjSTATE_PHYSICS), (1 << 13) - 1]:
    n = mj.mj_stateSize(m, sig)
    assert n == sum(v for b, v in sizes.items() if sig & b)
    assert p.get_state(sig).shape[-1] == n
  assert mj.mj_stateSize(m, int(mj.mjtState.mjSTATE_PHYSICS)) == c.nq + c.nv + c.na
  # sig = 0: an empty state through the seam, refused by the Physics facade; one bit too many: refused by both
  assert mj.mj_stateSize(m, 0) == 0
  with pytest.raises(ValueError):
    p.get_state(0)
  with pytest.raises(mj.FatalError):
    mj.mj_stateSize(m, 1 << 13)
  with pytest.raises(ValueError):
    p.get_state(1 << 13)
  p.free()


def test_create_batch_falls_back_through_the_contact_capacities():
  calls = []

  def factory(fits, error='scratch of %d contacts does not fit in LDS'):
    def make(model, batch_size, nconmax, **kw):
      calls.append(nconmax)
      if nconmax not in fits:
        raise RuntimeError(error % nconmax)
      return (model, batch_size, nconmax, kw)
    return make
  assert host_data.create_batch(factory((32, 0)), 'm', 5, precision=64) == ('m', 5, 32, dict(precision=64))
  assert calls == [64, 48, 32] == list(host_data.AUTO_NCONMAX[:3])
  del calls[:]
  with pytest.raises(RuntimeError, match='out of memory 64'):      # any other error: from the first call
    host_data.create_batch(factory((), 'out of memory %d'), 'm', 1)
  assert calls == [64]
  del calls[:]
  with pytest.raises(RuntimeError, match='0 contacts does not fit'):      # the last capacity's error is the caller's
    host_data.create_batch(factory(()), 'm', 1)
  assert calls == [64, 48, 32, 0]


def test_send_xfrc_holds_zeros_back_until_a_wrench_was_sent():
  state = {}
  zeros, wrench = np.zeros((2, 6)), np.eye(2, 6)
  assert not host_data.send_xfrc(state, zeros) and not state      # nothing to clear yet
  assert host_data.send_xfrc(state, wrench)
  assert host_data.send_xfrc(state, zeros)                        # ... now there is
  assert not host_data.send_xfrc({}, zeros)                       # another batch: its own history

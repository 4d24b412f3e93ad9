"""The C ABI's field table on the device: every data field of include/dmc_model_layout.h (dm_control_amd/_layout.py) has
the evaluated rows, round-trips exactly through every transfer path, keeps its error texts; a Field outlives
dmc_batch_set_env_geoms; one step still matches the oracle."""
import ctypes
import os

import numpy as np
import pytest

import data_fields_model
from dm_control_amd import _layout, mjcf_compiler as mc
from test_gpu_parity import TOL_F64_1000, _oracles, _rel_err

pytestmark = pytest.mark.gpu

REAL = [n for n, _ in _layout.DATA_REAL_FIELDS]
INT = [n for n, _ in _layout.DATA_INT_FIELDS]
# B = 3: a ragged wave, less than one 32-wide transposition tile; B = 33 crosses a tile edge
SHAPES = [(3, 32), (3, 64), (33, 32), (33, 64)]


def _batch(model, B, precision, **kw):
  from dm_control_amd.batch import BatchedPhysics
  return BatchedPhysics(model, B, precision=precision, **kw)


def _values(B, rows, shift=0.0):
  """env * 1000 + row (+ shift): exactly representable in fp32."""
  return np.arange(B)[:, None] * 1000.0 + np.arange(rows)[None, :] + shift


@pytest.fixture(scope='module')
def small():
  return data_fields_model.model()


@pytest.fixture(scope='module', params=SHAPES, ids=lambda p: 'B%d-fp%d' % p)
def batch(request, small):
  B, precision = request.param
  b = _batch(small, B, precision, nconmax=data_fields_model.NCONMAX)
  yield b
  b.close()


def test_rows_of_every_field(batch, small):
  assert batch.info()['nconmax'] == data_fields_model.NCONMAX
  counts = _layout.data_field_counts(small, data_fields_model.NCONMAX)
  assert counts['mocap_pos'] == 3 and counts['act'] == 1 and counts['contact_dist'] == 4
  for names, is_int in ((REAL, False), (INT, True)):
    for n in names:
      assert batch._rows(n) == (counts[n], is_int), n


def test_set_then_get_returns_every_field_exactly(batch):
  B = batch.batch_size
  for n in REAL + INT:
    want = _values(B, batch._rows(n)[0])
    batch.set(n, want)
    got = batch.get(n)
    assert got.dtype == (np.int32 if n in INT else np.float64)
    np.testing.assert_array_equal(got, want, err_msg=n)


@pytest.mark.parametrize('host', [np.float32, np.float64])
def test_async_transfers_of_four_fields_equal_the_synchronous_ones(batch, host):
  B, names = batch.batch_size, ('qpos', 'xfrc_applied', 'time', 'mocap_quat')
  want = {n: _values(B, batch._rows(n)[0], 0.5) for n in names}
  for n in names:
    batch.set_async(n, want[n].astype(host))
  batch.get_async(names)
  got = batch.get_wait(dtype=host)
  for n in names:
    assert got[n].dtype == host
    np.testing.assert_array_equal(got[n], want[n], err_msg=n)
    np.testing.assert_array_equal(got[n], batch.get(n).astype(host), err_msg=n)


def test_unknown_names_keep_their_error_texts(batch):
  from dm_control_amd import _native
  L, buf = _native.lib(), np.zeros((batch.batch_size, 64))
  for call, name, text in ((lambda n: L.dmc_batch_field_rows(batch._ptr, n, None, None), b'nope', 'unknown field: nope'),
                           (lambda n: L.dmc_batch_bind(batch._ptr, n, None), b'env_geom', 'unknown field: env_geom'),
                           (lambda n: L.dmc_batch_get(batch._ptr, n, buf.ctypes.data), b'ncon', 'unknown real field: ncon'),
                           (lambda n: L.dmc_batch_set(batch._ptr, n, buf.ctypes.data), b'nope', 'unknown real field: nope'),
                           (lambda n: L.dmc_batch_set_async(batch._ptr, n, buf.ctypes.data, 64, None), b'warning', 'unknown real field: warning'),
                           (lambda n: L.dmc_batch_get_int(batch._ptr, n, buf.ctypes.data), b'qpos', 'unknown int field: qpos'),
                           (lambda n: L.dmc_batch_set_int(batch._ptr, n, buf.ctypes.data), b'nope', 'unknown int field: nope')):
    assert call(name) == -1
    assert L.dmc_last_error().decode() == text
  arr = (ctypes.c_char_p * 2)(b'qpos', b'nope')
  assert L.dmc_batch_get_async(batch._ptr, 2, arr, None) == -1
  assert L.dmc_last_error().decode() == 'unknown field: nope'


def test_fields_without_rows_get_and_set_without_error():
  from dm_control_amd import _native
  with open(os.path.join(os.path.dirname(mc.__file__), 'suite', 'assets', 'cheetah.xml')) as f:
    m = mc.compile_xml(f.read())
  b, L = _batch(m, 3, 32), _native.lib()
  buf = np.full((3, 4), 7.0)
  for n in (b'act', b'mocap_pos'):
    assert b._rows(n.decode()) == (0, False)
    _native.check(L.dmc_batch_set(b._ptr, n, buf.ctypes.data))
    _native.check(L.dmc_batch_set_async(b._ptr, n, buf.ctypes.data, 32, None))
    _native.check(L.dmc_batch_get(b._ptr, n, buf.ctypes.data))
  got = b.get_many(('act', 'qpos', 'mocap_pos'))
  assert got['act'].shape == (3, 0) and got['mocap_pos'].shape == (3, 0)
  np.testing.assert_array_equal(got['qpos'], np.tile(m.qpos0, (3, 1)))
  assert (buf == 7.0).all()
  b.close()


@pytest.mark.parametrize('precision', [32, 64])
def test_an_enqueued_get_survives_the_declaration_of_env_geoms(small, precision):
  """The get's record points at the batch's fields; declaring the per-environment geoms adds one while it is in flight."""
  b = _batch(small, 33, precision, nconmax=data_fields_model.NCONMAX)
  want = _values(33, small.nq)
  b.set('qpos', want)
  b.get_async(('qpos',))
  b.set_env_geoms(['floor'])
  np.testing.assert_array_equal(b.get_wait()['qpos'], want)
  assert b._rows('env_geom') == (16, False)
  np.testing.assert_array_equal(b.get('qpos'), want)
  b.close()


@pytest.mark.parametrize('B', [3, 33])
def test_one_step_matches_the_oracle_in_fp64(small, B):
  from oracle import oracle
  m = small
  rs = np.random.RandomState(B)
  q = np.tile(m.qpos0, (B, 1)) + np.stack([np.linspace(-.01, .02, B), rs.uniform(-1, 1, B)], 1)      # the box from 1 cm in the floor to 2 cm above it, tilted
  v, c = rs.uniform(-1, 1, (B, m.nv)), rs.uniform(-1, 1, (B, m.nu))
  b = _batch(m, B, 64, nconmax=data_fields_model.NCONMAX)
  b.set('qpos', q); b.set('qvel', v); b.set('ctrl', c)
  refs = _oracles(m, q, v)
  b.step()
  oracle.rollout_legacy(refs, c[None])
  qo = np.stack([p.qpos for p in refs])
  err = _rel_err(b.get('qpos'), qo)
  print('one-step fp64 rel qpos error vs oracle, B = %d: %.3e' % (B, err))
  assert (b.get('ncon') > 0).any() and np.abs(qo - q).max() > 1e-4
  assert err < TOL_F64_1000
  np.testing.assert_allclose(b.get('act'), np.stack([p.act for p in refs]), rtol=0, atol=TOL_F64_1000)
  b.close()

"""CPU tier of the batched dynamics (dm_control_amd/dynamics.py, csrc/dyn_core.h): the host build of the device header in
both real types against the fp64 oracle's qM / qfrc_bias / qfrc_smooth and host_data.mass_matrix on every model of
tests/dynamics_cases.py; symmetry and sparsity of M to the bit; equal bits at every number of lanes per environment; the
gravity flag; the pivot clamp; the refusals; host_data.rne and the host seam's mj_rne / mj_mulM / mj_solveM; the
sanitizers on a stand-alone program."""
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

import dyn_emu_lib as emu      # noqa: E402
import dynamics_cases as dc      # noqa: E402
from dm_control_amd import dynamics      # noqa: E402
from dm_control_amd import host_data      # noqa: E402

NSTATES = {'fixture': dc.NSTATE, 'fixture_nogravity': dc.NSTATE}      # the suite models and the mocap model: 4 states each


@pytest.fixture(scope='module')
def world():
  """Per model: dict(m, tables, qpos, qvel, qacc, vec, ref): the oracle's references of every state, computed once."""
  w = {}
  for name in dc.MODELS:
    m = dc.model(name)
    n = NSTATES.get(name, 4)
    qpos, qvel = dc.states(m, n)
    qacc, vec = dc.inputs(m.nv, n)
    w[name] = dict(m=m, tables=dynamics.model_tables(m), qpos=qpos, qvel=qvel, qacc=qacc, vec=vec,
                   ref=[dc.reference(m, qpos[s], qvel[s], qacc[s], vec[s]) for s in range(n)])
  return w


def test_models_exercise_every_path(world):
  m = world['fixture']['m']
  assert m.nv == 62 and m.nbody == 15 and {0, 1, 2, 3} <= {int(t) for t in m.jnt_type}
  assert float(m.opt.gravity[2]) == -9.81 and np.all(np.asarray(m.dof_armature) == 0.01) and np.all(np.asarray(m.dof_damping) == 0.1)
  d = world['fixture']['tables']['dims']
  assert (d['nb'], d['nv'], d['nlevel']) == (15, 62, 6)
  # no contact in 14 of the 16 states; in states 6 and 12 a box touches the arm (dynamics_cases.CONTACT_STATES).  The references
  # do not depend on it: qacc_smooth and qfrc_smooth are the oracle's values BEFORE the constraint solve (held below)
  assert {s: r['ncon'] for s, r in enumerate(world['fixture']['ref']) if r['ncon']} == dc.CONTACT_STATES
  assert max(np.linalg.cond(r['M']) for r in world['fixture']['ref']) <= 1.2e3
  assert max(np.abs(r['bias']).max() for r in world['fixture']['ref']) <= 98
  assert [dynamics.choose_lanes(world[n]['tables']['dims']['nb'], world[n]['m'].nv, 32) for n in ('cheetah', 'humanoid', 'humanoid_CMU')] == [16, 32, 64]
  # the mocap body and what is welded to it are left out; the static base of the arm is kept (the arm's frame hangs off it)
  mo = world['mocap']
  names = mo['m'].names['body']
  assert [names[b] for b in mo['tables']['bodies']] == ['world', 'base', 'arm', 'fore', 'puck'] and mo['m'].nmocap == 1
  assert world['humanoid_CMU']['tables']['dims']['nlevel'] >= 8      # a deep tree
  # the oracle's own consistency: M qacc_smooth = qfrc_smooth (+ bias on both sides)
  for r in world['fixture']['ref']:
    assert np.abs(r['M'] @ r['qacc_smooth'] + r['bias'] - r['inverse_smooth']).max() <= 1e-12
    assert np.abs(r['M'] - r['M_host']).max() <= 1e-14


def test_host_build_meets_the_bounds_on_every_model(world):
  worst = {p: dict.fromkeys(dc.OUTPUTS + ('solve_forward', 'M_host', 'inverse_smooth'), 0.0) for p in (64, 32)}
  failed = []
  for name, w in world.items():
    for s, ref in enumerate(w['ref']):
      for prec in (64, 32):
        got = emu.run(prec, w['tables'], w['qpos'][s], w['qvel'][s], w['qacc'][s], w['vec'][s])
        err = dc.errors(got, ref, w['vec'][s])
        # M against host_data.mass_matrix too; inverse at qacc_smooth against qfrc_smooth + qfrc_bias
        err['M_host'] = float(np.abs(got['M'] - ref['M_host']).max() / max(1.0, np.abs(ref['M_host']).max()))
        sm = emu.run(prec, w['tables'], w['qpos'][s], w['qvel'][s], ref['qacc_smooth'], what=('inverse',))['inverse']
        err['inverse_smooth'] = float(np.abs(sm - ref['inverse_smooth']).max() / max(1.0, np.abs(ref['inverse_smooth']).max()))
        for k, v in err.items():
          worst[prec][k] = max(worst[prec][k], v)
          key = {'M_host': 'M', 'solve_forward': 'solve'}.get(k, k)
          if prec == 32 and k == 'solve_forward':
            continue      # (fp32: the backward error is what is judged)
          if prec == 64 and k == 'solve':
            continue      # (fp64: the forward error is)
          if v > dc.bound(prec, key):
            failed.append((name, s, prec, k, v))
  for prec in (64, 32):
    print('fp%d host build, worst error / max(1, |ref|max): %s' % (prec, ', '.join('%s %.3g' % kv for kv in worst[prec].items())))
  assert not failed, failed[:8]
  # the bounds are 4 x what this test measures (tests/dynamics_cases.py): the recorded values are the measured ones
  for k in dc.F32_MEASURED:
    m32 = max(worst[32][k], worst[32]['M_host'] if k == 'M' else 0)
    assert m32 <= dc.F32_MEASURED[k] <= 1.5 * m32, (k, m32, dc.F32_MEASURED[k])


def test_mass_matrix_is_symmetric_to_the_bit_and_zero_off_the_ancestor_paths(world):
  for name in ('fixture', 'humanoid_CMU', 'mocap'):
    w = world[name]
    m = w['m']
    par = [int(p) for p in m.dof_parentid]
    related = np.eye(m.nv, dtype=bool)
    for i in range(m.nv):
      j = par[i]
      while j >= 0:
        related[i, j] = related[j, i] = True
        j = par[j]
    for prec in (64, 32):
      M = emu.run(prec, w['tables'], w['qpos'][1], what=('M',))['M']
      assert np.array_equal(M, M.T)
      assert not M[~related].any()
      assert np.all(np.linalg.eigvalsh(M) > 0)


def test_fp64_results_do_not_depend_on_the_lanes_per_environment(world):
  for name in ('fixture', 'cheetah', 'humanoid_CMU'):
    w = world[name]
    for s in (0, 3):
      runs = [emu.run(64, w['tables'], w['qpos'][s], w['qvel'][s], w['qacc'][s], w['vec'][s], lanes=l) for l in (1, 16, 32, 64)]
      for r in runs[1:]:
        for k in dc.OUTPUTS:
          assert np.array_equal(r[k], runs[0][k]), (name, s, k)
  # (fp32 too: nothing in the header depends on the width)
  w = world['fixture']
  a, b = (emu.run(32, w['tables'], w['qpos'][0], w['qvel'][0], w['qacc'][0], w['vec'][0], lanes=l) for l in (16, 64))
  assert all(np.array_equal(a[k], b[k]) for k in dc.OUTPUTS)


def test_bias_without_gravity_at_rest_is_exactly_zero(world):
  w = world['fixture_nogravity']
  assert not w['tables']['gravity'].any() and float(w['m'].opt.gravity[2]) == -9.81
  for prec in (64, 32):
    for s in range(4):
      assert not emu.run(prec, w['tables'], w['qpos'][s], np.zeros(w['m'].nv), what=('bias',))['bias'].any()
  g = world['fixture']
  assert np.abs(emu.run(64, g['tables'], g['qpos'][0], np.zeros(62), what=('bias',))['bias']).max() > 1      # (with gravity: not zero)


def test_pivot_clamp_keeps_a_massless_leaf_finite(world):
  """The hand made massless and its hinge's armature removed: M(h3, h3) = 0, the pivot is replaced by mjMINVAL."""
  w = world['fixture']
  m = w['m']
  tb = dict(w['tables'])
  hand, h3 = m.name2id('hand', 'body'), int(m.jnt_dofadr[m.name2id('h3', 'joint')])
  d = tb['dims']
  reals = tb['reals'].copy()
  nb, nj = d['nb'], d['nj']
  assert tb['bodies'][hand] == hand
  reals[14*nb + hand] = 0                          # body_mass
  reals[15*nb + 3*hand:15*nb + 3*hand + 3] = 0     # body_inertia
  arm = 18*nb + 7*nj
  assert reals[arm + h3] == 0.01
  reals[arm + h3] = 0
  tb['reals'] = reals
  for prec in (64, 32):
    r = emu.run(prec, tb, w['qpos'][0], w['qvel'][0], w['qacc'][0], w['vec'][0])
    assert abs(r['M'][h3, h3]) < host_data.MINVAL
    assert all(np.all(np.isfinite(r[k])) for k in dc.OUTPUTS)
    assert np.abs(np.delete(r['solve'], h3, axis=1)).max() < 1e6      # the other dofs do not feel the clamped one


def test_refusals_are_loud(world):
  import torch
  from dm_control_amd import mjcf_compiler as mc
  with pytest.raises(TypeError, match='BatchedPhysics'):
    dynamics.BatchDynamics(object())
  still = mc.compile_xml('<mujoco><worldbody><body><geom size=".1"/></body></worldbody></mujoco>')
  with pytest.raises(ValueError, match='nv = 0'):
    dynamics.model_tables(still)
  below = mc.compile_xml('<mujoco><worldbody><body name="m" mocap="true"><geom size=".1"/><body name="stuck" pos="0 0 1"><geom size=".1"/>'
                         '<body name="swing"><joint name="j"/><geom size=".1"/></body></body></body></worldbody></mujoco>')
  with pytest.raises(ValueError, match="'swing'.*mocap"):
    dynamics.model_tables(below)
  for bad in (8, 48, -16, 128, 16.0, '32', None, True):
    with pytest.raises(ValueError, match='lanes_per_env'):
      dynamics.choose_lanes(8, 9, 32, bad)
  d = world['fixture']['tables']['dims']
  with pytest.raises(ValueError, match='too small for the model'):
    dynamics.choose_lanes(d['nb'], d['nv'], 64, 16)
  assert dynamics.choose_lanes(d['nb'], d['nv'], 64, 64) == 64 and dynamics.choose_lanes(d['nb'], d['nv'], 64) == 64
  assert dynamics.choose_lanes(d['nb'], d['nv'], 32, 32) == 32
  c = emu.caps(d['nb'], d['nv'], 16)
  assert (c['ws0'], c['ws1']) == (dynamics.workspace_reals(d['nb'], d['nv'], 0), dynamics.workspace_reals(d['nb'], d['nv'], 1))
  assert c['tier64'] == -1 and emu.caps(d['nb'], d['nv'], 64)['tier64'] == 2      # the header refuses what choose_lanes refuses
  # inputs: a stand-in for the object (no device here), the checks run before anything is launched
  bd = dynamics.BatchDynamics.__new__(dynamics.BatchDynamics)
  bd.batch, bd.nv = types.SimpleNamespace(device_id=0, precision=64, batch_size=4), 5
  with pytest.raises(ValueError, match='dtype'):
    bd._input(torch.zeros(4, 5, dtype=torch.float32), ((4, 5),), 'v')
  with pytest.raises(ValueError, match='expected a tensor on cuda'):
    bd._input(torch.zeros(4, 5, dtype=torch.float64), ((4, 5),), 'v')
  for shape in ((4, 6), (3, 5), (4, 2, 6), (5,), (4, 5, 1, 1)):
    with pytest.raises(ValueError, match='shape'):
      bd._input(np.zeros(shape), ((4, 5), (4, None, 5)), 'v')
  with pytest.raises(ValueError, match='K = 0'):
    bd._input(np.zeros((4, 0, 5)), ((4, 5), (4, None, 5)), 'f')
  with pytest.raises(ValueError, match='real numbers'):
    bd._input(np.zeros((4, 5), dtype=complex), ((4, 5),), 'v')
  with pytest.raises(ValueError, match='shape'):
    bd.inverse(np.zeros((4, 6)))
  for call in (bd.mul, bd.solve):
    with pytest.raises(ValueError, match='K = 0'):
      call(np.zeros((4, 0, 5)))


def test_host_rne_and_the_seam_agree_with_the_oracle(world, monkeypatch):
  import oracle_backend as ob
  from dm_control_amd import mujoco_api as mj
  from oracle.oracle import OraclePhysics
  for name in ('fixture', 'humanoid', 'mocap', 'fixture_nogravity'):
    w = world[name]
    m = w['m']
    for s in range(2):
      ref = w['ref'][s]
      p = OraclePhysics(m)
      p.qpos[:] = w['qpos'][s]
      p.qvel[:] = w['qvel'][s]
      p.forward()
      g = lambda n, *sh: np.array(p.field(n), dtype=np.float64).reshape(*sh)
      poses = (g('xpos', -1, 3), g('xquat', -1, 4), g('xipos', -1, 3), g('ximat', -1, 9))
      for qacc, key in ((None, 'bias'), (w['qacc'][s], 'inverse'), (ref['qacc_smooth'], 'inverse_smooth')):
        got = host_data.rne(m, w['qpos'][s], w['qvel'][s], qacc, *poses)
        assert np.abs(got - ref[key]).max() <= dc.F64_TOL * max(1.0, np.abs(ref[key]).max()), (name, s, key)
  # the seam: one environment of host numpy on the oracle
  monkeypatch.setattr(mj, 'BatchedPhysics', ob.OracleBatch)
  w = world['fixture']
  s, nv = 2, 62
  ref = w['ref'][s]
  mm = mj.MjModel.from_xml_string(dc.xml())
  dd = mj.MjData(mm)
  dd.qpos[:] = w['qpos'][s]
  dd.qvel[:] = w['qvel'][s]
  mj.mj_forward(mm, dd)
  tol = lambda r: dc.F64_TOL * max(1.0, np.abs(r).max())
  out = np.full(nv, np.nan)
  mj.mj_rne(mm, dd, 0, out)
  assert np.abs(out - ref['bias']).max() <= tol(ref['bias'])
  mj.mj_rne(mm, dd, 1, out)
  full = ref['M'] @ np.asarray(dd.qacc) + ref['bias']
  assert np.abs(out - full).max() <= tol(full)
  mj.mj_mulM(mm, dd, out, w['vec'][s][0])
  assert np.abs(out - ref['mul'][0]).max() <= tol(ref['mul'])
  x = np.full((dc.K, nv), np.nan)
  mj.mj_solveM(mm, dd, x, w['vec'][s], dc.K)
  assert np.abs(x - ref['solve']).max() <= tol(ref['solve'])
  y = w['vec'][s][1].copy()
  mj.mj_solveM(mm, dd, y, y, 1)      # in place
  assert np.abs(y - ref['solve'][1]).max() <= tol(ref['solve'])
  dense = np.zeros((nv, nv))
  mj.mj_fullM(mm, dense, dd.qM)
  assert np.abs(dense - ref['M']).max() <= tol(ref['M'])
  for bad in (lambda: mj.mj_rne(mm, dd, 0, np.zeros(nv + 1)), lambda: mj.mj_mulM(mm, dd, np.zeros(nv), np.zeros(nv - 1)),
              lambda: mj.mj_solveM(mm, dd, np.zeros((2, nv)), np.zeros((2, nv)), 3)):
    with pytest.raises(mj.FatalError):
      bad()


def test_native_entry_points_validate_without_a_device():
  from dm_control_amd import build
  build.build()
  from dm_control_amd import _native
  with open(os.path.join(ROOT, 'include', 'dmc_dyn.h')) as f:
    declared = set(re.findall(r'\b(dmc_dyn_[a-z0-9_]+)\s*\(', f.read()))
  assert declared == set(_native.DYN_EXPORTS)
  L = _native.lib()
  assert not [n for n in sorted(declared) if not hasattr(L, n)]
  out = ctypes.c_void_p()
  buf = (ctypes.c_double * 16)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  assert L.dmc_dyn_create(None, p, 64, ctypes.byref(out)) != 0 and b'null' in L.dmc_last_error() and not out.value
  assert L.dmc_dyn_mass_matrix(None, p, None) != 0 and b'null' in L.dmc_last_error()
  assert L.dmc_dyn_bias(None, p, None) != 0 and L.dmc_dyn_inverse(None, p, 0, p, None) != 0
  assert L.dmc_dyn_mul(None, p, 1, p, None) != 0 and L.dmc_dyn_solve(None, p, 1, p, None) != 0
  assert L.dmc_dyn_mul(p, p, 0, p, None) != 0 and b'at least one' in L.dmc_last_error()
  assert L.dmc_dyn_solve(p, p, 0, p, None) != 0 and b'at least one' in L.dmc_last_error()
  assert L.dmc_dyn_info(None, p) != 0
  L.dmc_dyn_destroy(None)
  units = {u[0]: u for u in build._UNITS}
  assert 'dyn_core.h' in units['dyn_kernels.hip'][2] and 'jac_core.h' in units['dyn_kernels.hip'][2] and '-ffp-contract=off' in units['dyn_kernels.hip'][1]
  c = emu.caps(33, 64, 64)      # nv = 64 with 32 bodies: the static LDS holds it in both precisions
  assert c['max_dofs'] == dynamics.MAX_DOFS == 64 and c['block'] == 64 and c['chunk'] == dynamics.CHUNK
  assert c['tier64'] == 2 and c['tier32'] >= 0 and 8 * c['ws0'] <= 65536
  for src in ('dyn_core.h', 'dyn_kernels.hip'):
    with open(os.path.join(build.CSRC, src)) as f:
      text = f.read()
    assert not re.search(r'\basm\b|__asm|atomic[A-Z_(]', text)      # plain arithmetic: no assembly, no atomic call


def test_sanitized_stand_alone_program_over_the_cases(tmp_path, world):
  """csrc/dyn_core.h under AddressSanitizer and UBSan: a program with its own main (tests/emu/dyn_sanitize.cpp), fed the
  tables and the states as text, in both precisions and at 16 and 64 lanes -- never through Python, never on a GPU."""
  exe = str(tmp_path / 'dyn_sanitize')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                         '-Wno-unknown-pragmas', '-o', exe, os.path.join(ROOT, 'tests', 'emu', 'dyn_sanitize.cpp')])
  num = lambda a: ' '.join(repr(float(x)) for x in np.asarray(a).ravel())
  for name, ncase in (('fixture', 4), ('mocap', 4), ('humanoid_CMU', 2)):
    w = world[name]
    tb, nv = w['tables'], w['m'].nv
    lines = [' '.join(str(int(x)) for x in emu.dims_array(tb)) + ' %d %d' % (dc.K, ncase), ' '.join(str(int(x)) for x in tb['ints']), num(tb['reals'])]
    for s in range(ncase):
      lines.append(' '.join(num(w[k][s]) for k in ('qpos', 'qvel', 'qacc', 'vec')))
    res = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120, check=False)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [np.array([float(x) for x in l.split()]) for l in res.stdout.strip().split('\n')]
    assert len(rows) == 4 * ncase and all(r.shape == (1 + 2*nv + 2*dc.K*nv,) for r in rows)
    for s in range(ncase):
      for i, prec in enumerate((64, 32)):
        r = emu.run(prec, tb, w['qpos'][s], w['qvel'][s], w['qacc'][s], w['vec'][s])
        want = np.concatenate([r['bias'], r['inverse'], r['mul'].ravel(), r['solve'].ravel()])
        for lanes in range(2):      # (-O1 against the library's -O2, both without contraction: the same IEEE operations)
          got = rows[4*s + 2*i + lanes]
          np.testing.assert_array_equal(got[1:], want)
          assert abs(got[0] - np.abs(r['M']).sum()) <= 1e-12 * max(1, got[0])

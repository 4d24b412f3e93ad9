"""Batched geom distances, CPU tier: the fp64 twin (tests/dist_twin.py, written from the definition) against closed forms
and against the unchanged fp64 oracle's contact records; the host build of the solver (tests/emu/dist_emu.cpp:
csrc/dist_core.h in fp32 and fp64) against the twin over the fixture tests/golden/distance_cases.npz; the library's host
entry and mujoco_api.mj_geomDistance on the oracle stand-in; pairs_from_sensors; and what BatchDistance / proximity.wrap
check before they touch a device.

Measured (scripts/make_distance_golden.py, profiles/distance_accuracy.json): e_twin 1.9e-14; fp64 host build against the
twin 9.6e-7 over all pairs (the bound is the solver's own gap, 1e-6 max(1, |d|)) and 4.4e-16 over the pairs whose cores
are points, segments or boxes; fp32 host build 3.75e-6."""
import collections
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import dist_emu_lib as emu
import dist_twin as tw
import distance_cases as dc
from dm_control_amd import distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM = slice(0, dc.NSTATE)


@pytest.fixture(scope='module')
def golden():
  return dc.load_golden()


@pytest.fixture(scope='module')
def solved(golden):
  """The host build over every case of the fixture, per precision: computed once, shared."""
  out = {}
  for prec in (64, 32):
    rows = []
    for s in range(len(golden['pos'])):
      G = dc.geoms_of(golden['pos'][s], golden['quat'][s])
      rows.append(emu.pairs(prec, [G[p[0]] for p in dc.PAIRS], [G[p[1]] for p in dc.PAIRS], dc.DISTMAX, dc.TOLERANCE, dc.ITERATIONS))
    out[prec] = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
  return out


def dist_bound(prec, ref):
  """(S, P) bounds on |d - d_twin|: the issue's rule per pair."""
  scale = np.maximum(1.0, np.abs(ref))
  if prec == 32:
    return dc.F32_TOL*scale
  exact = np.array([dc.exact_pair(p) for p in dc.PAIRS])
  return np.where(exact, dc.TOL_F64*scale, dc.TOLERANCE*scale + dc.E_TWIN)


def test_fixture_is_what_the_live_twin_computes(golden):
  pos, quat, aligned = dc.states()
  assert np.array_equal(pos, golden['pos']) and np.array_equal(quat, golden['quat']) and np.array_equal(aligned, golden['aligned'])
  assert golden['dist'].shape == (dc.NSTATE + 5, 55) and os.path.getsize(dc.GOLDEN) < 400*1024
  rs = np.random.RandomState(5)
  picks = [(int(s), int(p)) for s, p in zip(rs.randint(0, len(pos), 10), rs.randint(0, 55, 10))] + [(33, 54), (0, 30)]
  kinds = set()
  for s, pi in picks:
    d, ft, unique, gap = dc.twin_case(dc.geoms_of(pos[s], quat[s]), dc.PAIRS[pi])
    kinds.add(d > 0)
    assert abs(d - golden['dist'][s, pi]) <= 1e-12 and np.max(np.abs(ft - golden['fromto'][s, pi])) <= 1e-9
    assert (unique and not aligned[s]) == golden['unique'][s, pi]
  assert kinds == {True, False}


def test_class_mix_and_unique_share_from_the_twin_alone(golden):
  mix, left_out = collections.defaultdict(collections.Counter), collections.Counter()
  for pi, p in enumerate(dc.PAIRS):
    for s in range(dc.NSTATE):
      mix[dc.type_pair(p)][dc.classify(p, golden['dist'][s, pi])] += 1
      left_out[dc.type_pair(p)] += not golden['unique'][s, pi]
  assert len(mix) == 20
  for tp, c in mix.items():
    n = sum(c.values())
    assert n in (32, 64, 128) and set(c) <= set(dc.classes_allowed(tp))
    for k in dc.classes_allowed(tp):
      assert c[k] >= dc.MIX_MIN*n, (tp, k, c)
    assert left_out[tp] <= dc.UNIQUE_CAP*n, (tp, left_out[tp])
  assert not golden['unique'][dc.NSTATE:].any()      # the axis-aligned states are never compared point for point


def test_twin_against_closed_forms(golden):
  worst, seen = 0.0, collections.Counter()
  for s in range(len(golden['pos'])):
    G = dc.geoms_of(golden['pos'][s], golden['quat'][s])
    for pi, p in enumerate(dc.PAIRS):
      if tw.PLANE in dc.type_pair(p):
        cf = G[p[1]].pos[2] - GEOM_LOW[G[p[1]].type](G[p[1]]) if G[p[1]].type in GEOM_LOW else None
      else:
        cf = tw.closed_form(G[p[0]], G[p[1]])
      if cf is not None:
        seen[dc.type_pair(p)] += 1
        worst = max(worst, abs(cf - golden['dist'][s, pi])/max(1.0, abs(cf)))
  assert set(seen) >= {(0, 2), (2, 2), (2, 3), (3, 3), (2, 6), (6, 6)} and seen[(6, 6)] >= 10
  assert worst <= 4*dc.E_TWIN
  assert golden['gap'].max() <= 4*dc.E_TWIN      # the twin's own primal-dual gap where the geoms are apart


GEOM_LOW = {tw.SPHERE: lambda g: g.size[0]}      # sphere-plane: height of the centre minus the radius


def test_twin_equals_the_oracles_contact_distances(golden):
  """The oracle's contact records inside a 1 m margin: min dist over the pair's contacts, for the pair types whose
  collider returns the geometric distance (dc.ORACLE_PIN_TYPES); the witness points pos -/+ dist normal / 2 where the
  pair has one contact and the twin marks the witness unique."""
  from dm_control_amd import mjcf_compiler as mc
  from oracle.oracle import OraclePhysics
  m = mc.compile_xml(dc.xml(margin=1.0))
  seen, points = collections.Counter(), 0
  for s in (2, 3, 7, 8, 13):
    p = OraclePhysics(m)
    p.qpos[:] = dc.qpos_of(golden['pos'][s], golden['quat'][s])
    p.forward()
    per_pair = collections.defaultdict(list)
    for i in range(int(p.ncon)):
      c = p.contact(i)
      per_pair[(min(c['geom1'], c['geom2']), max(c['geom1'], c['geom2']))].append(c)
    for pi, pr in enumerate(dc.PAIRS):
      if dc.type_pair(pr) not in dc.ORACLE_PIN_TYPES or pr not in per_pair:
        continue
      c = min(per_pair[pr], key=lambda c: c['dist'])
      d = golden['dist'][s, pi]
      assert abs(c['dist'] - d) <= dc.TOL_F64*max(1.0, abs(d)), (s, pr, c['dist'], d)
      seen[dc.type_pair(pr)] += 1
      if len(per_pair[pr]) == 1 and golden['unique'][s, pi] and c['geom1'] == pr[0]:
        n = c['frame'][0]
        ft = np.concatenate([c['pos'] - 0.5*c['dist']*n, c['pos'] + 0.5*c['dist']*n])
        assert np.max(np.abs(ft - golden['fromto'][s, pi])) <= dc.WITNESS_TOL[64], (s, pr)
        points += 1
  assert set(seen) == set(dc.ORACLE_PIN_TYPES) and points >= 50


@pytest.mark.parametrize('prec', [64, 32])
def test_every_case_converges_at_the_default_options(solved, prec):
  assert not solved[prec]['status'].any()
  assert solved[prec]['epa'].sum() >= 400      # (and EPA is what a quarter of them ran)


@pytest.mark.parametrize('prec', [64, 32])
def test_dist_against_the_twin(golden, solved, prec):
  ref = np.minimum(golden['dist'], dc.DISTMAX)
  err = np.abs(solved[prec]['dist'] - ref)
  print('fp%d worst |d - twin| / max(1, |d|): %.3e' % (prec, np.max(err/np.maximum(1.0, np.abs(ref)))))
  assert np.all(err <= dist_bound(prec, ref))


@pytest.mark.parametrize('prec', [64, 32])
def test_fromto_and_normal_invariants(golden, solved, prec):
  r = solved[prec]
  near = r['dist'] < dc.DISTMAX
  assert near.sum() > 1900 and not r['fromto'][~near].any() and not r['normal'][~near].any()
  frm, to, n, d = r['fromto'][..., :3], r['fromto'][..., 3:], r['normal'], r['dist']
  bound = dist_bound(prec, np.minimum(golden['dist'], dc.DISTMAX)) + (1e-6 if prec == 32 else 0)      # (+ fp32 rounding of a point's coordinates)
  assert np.all(np.abs(np.linalg.norm(to - frm, axis=-1) - np.abs(d))[near] <= bound[near])
  assert np.all(np.abs(np.linalg.norm(n, axis=-1) - 1)[near] <= (1e-12 if prec == 64 else 1e-5))
  assert np.all((np.linalg.norm(to - frm - d[..., None]*n, axis=-1))[near] <= bound[near])      # the sign: to - from = dist normal
  worst = 0.0
  for s in range(len(d)):
    G = dc.geoms_of(golden['pos'][s], golden['quat'][s])
    for pi, p in enumerate(dc.PAIRS):
      if near[s, pi]:
        e = max(abs(G[p[0]].surface(frm[s, pi])), abs(G[p[1]].surface(to[s, pi])))
        worst = max(worst, e/bound[s, pi])
  print('fp%d worst surface residual / bound: %.3f' % (prec, worst))
  assert worst <= 1.0


@pytest.mark.parametrize('prec', [64, 32])
def test_fromto_against_the_twin_where_unique(golden, solved, prec):
  u = golden['unique']
  assert u[RANDOM].mean() >= 1 - dc.UNIQUE_CAP
  err = np.max(np.abs(solved[prec]['fromto'] - golden['fromto']), axis=-1)
  print('fp%d worst witness error where unique: %.3e' % (prec, err[u].max()))
  assert np.all(err[u] <= dc.WITNESS_TOL[prec])


def test_passed_over_seeds_report_status_1_within_their_own_gap():
  for k, seed, p in dc.STATUS1_CASES:
    G = dc.geoms_of(*dc.random_state(k, seed))
    d = tw.distance(G[p[0]], G[p[1]])['dist']
    for prec, slack in ((64, dc.E_TWIN + 1e-12), (32, dc.F32_TOL)):
      r = _one(G[p[0]], G[p[1]], prec)
      # fp64 must report the cap.  fp32 may report status 0 here and that is intended, not a loophole: status 0 certifies
      # max(tolerance, 128 machine epsilons) = 1.5e-5 in fp32 (PARITY row 65), and a fp32 solve that stops inside that
      # floor has converged by its own rule; the bracket below holds for it either way.
      assert r['epa'] == 1 and (r['status'] != 0 or prec == 32) and r['gap'] > dc.TOLERANCE
      print('fp%d state %d seed %d pair %s: status %d, dist - twin %.3e, certified gap %.3e' % (prec, k, seed, p, r['status'], r['dist'] - d, r['gap']))
      assert d - r['gap'] - slack <= r['dist'] <= d + slack      # an attained value: on the deep side, inside the certificate


def _one(a, b, prec=64, **kw):
  r = emu.pairs(prec, [a], [b], **kw)
  return {k: v[0] for k, v in r.items()}


def test_distmax_planes_swap_and_degenerate_pairs():
  I = np.eye(3)
  a, b = tw.Geom(tw.SPHERE, (0.1, 0, 0), (0, 0, 0), I), tw.Geom(tw.BOX, (0.1, 0.2, 0.3), (1.0, 0, 0), I)
  r = _one(a, b)
  assert r['dist'] == pytest.approx(0.8, abs=1e-12) and np.allclose(r['fromto'], [0.1, 0, 0, 0.9, 0, 0], atol=1e-12)
  assert np.allclose(r['normal'], [1, 0, 0], atol=1e-12)
  r = _one(a, b, distmax=0.5)      # nothing below distmax: distmax, zero fromto, zero normal
  assert r['dist'] == 0.5 and not r['fromto'].any() and not r['normal'].any() and r['status'] == 0
  pl = tw.Geom(tw.PLANE, (0, 0, 0.1), (0, 0, 0), I)
  r = _one(pl, tw.Geom(tw.PLANE, (0, 0, 0.1), (0, 0, 1), I), distmax=3.0)      # plane-plane has no collider
  assert r['dist'] == 3.0 and not r['fromto'].any()
  cap = tw.Geom(tw.CAPSULE, (0.05, 0.2, 0), (0.3, 0, 0.5), tw.quat_to_mat((0.9, 0.1, 0.4, 0)))
  r1, r2 = _one(pl, cap), _one(cap, pl)      # a plane on either side; infinite (the capsule is beyond the half-size 0)
  assert r1['dist'] == pytest.approx(r2['dist'], abs=1e-15) and r1['dist'] == pytest.approx(tw.distance(pl, cap)['dist'], abs=1e-12)
  assert np.allclose(r1['normal'], [0, 0, 1]) and np.allclose(r2['normal'], [0, 0, -1]) and abs(r1['fromto'][2]) < 1e-15
  # swapping geom1 and geom2 swaps from and to (over a spread of fixture pairs of every class)
  g = dc.load_golden()
  for s, pi in ((0, 20), (1, 33), (2, 48), (3, 54), (5, 12), (6, 40), (10, 25), (4, 50)):
    G = dc.geoms_of(g['pos'][s], g['quat'][s])
    x, y = G[dc.PAIRS[pi][0]], G[dc.PAIRS[pi][1]]
    f, b2 = _one(x, y), _one(y, x)
    tol = dc.TOLERANCE*max(1.0, abs(f['dist']))
    assert abs(f['dist'] - b2['dist']) <= tol
    if g['unique'][s, pi]:
      assert np.max(np.abs(f['fromto'][:3] - b2['fromto'][3:])) <= dc.WITNESS_TOL[64] and np.max(np.abs(f['fromto'][3:] - b2['fromto'][:3])) <= dc.WITNESS_TOL[64]
      assert np.max(np.abs(f['normal'] + b2['normal'])) <= 2*dc.WITNESS_TOL[64]
  # concentric spheres: the depth is the sum of the radii, the direction the solver's documented choice (+z)
  r = _one(a, tw.Geom(tw.SPHERE, (0.25, 0, 0), (0, 0, 0), I))
  assert r['dist'] == pytest.approx(-0.35, abs=1e-15) and r['status'] == 0 and np.allclose(r['normal'], [0, 0, 1])
  assert _one(pl, tw.Geom(tw.PLANE, (0, 0, 0.1), (0, 0, 1), I), distmax=np.inf)['dist'] == np.inf      # the default cutoff stays infinite
  # the iteration cap is reported, with a bound that still brackets the truth from above (dist is an attained value)
  e1, e2 = tw.Geom(tw.ELLIPSOID, (0.16, 0.10, 0.07), (0, 0, 0), I), tw.Geom(tw.ELLIPSOID, (0.09, 0.12, 0.15), (0.02, 0.01, 0.015), tw.quat_to_mat((0.8, 0.3, 0.1, 0.5)))
  r = _one(e1, e2, iterations=6)
  assert r['status'] != 0 and r['epa'] == 1 and r['dist'] <= tw.distance(e1, e2)['dist'] + 1e-9


def test_caps_fit_the_static_lds_limit():
  c = emu.caps()
  assert c['block'] == 64 and c['V32'] >= dc.ITERATIONS + 4 and c['V64'] >= dc.ITERATIONS + 4 and c['V64'] < 256
  assert c['F32'] >= 2*c['V32'] - 4 and c['F64'] >= 2*c['V64'] - 4
  for es, v, f, k in ((4, c['V32'], c['F32'], c['K32']), (8, c['V64'], c['F64'], c['K64'])):
    assert es*((3*v + f)*k + 15*64) + 4*f*k <= 65536 and k >= 16


def test_host_entry_and_mj_geom_distance_on_the_oracle_stand_in(golden, monkeypatch):
  import oracle_backend as ob
  from dm_control_amd import build, mujoco_api as mj
  build.build()
  from dm_control_amd import _native
  with open(os.path.join(ROOT, 'include', 'dmc_dist.h')) as f:
    declared = set(re.findall(r'\b(dmc_(?:dist|geom_distance)_[a-z0-9_]+)\s*\(', f.read()))
  assert declared == set(_native.DIST_EXPORTS)
  L = _native.lib()
  assert not [n for n in sorted(declared) if not hasattr(L, n)]
  out = ctypes.c_void_p()
  buf = (ctypes.c_double * 16)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  assert L.dmc_dist_create(None, 1, p, p, 2, p, p, ctypes.byref(out)) != 0 and b'null' in L.dmc_last_error() and not out.value
  assert L.dmc_dist_query(None, p, None, None, None, None) != 0 and b'null' in L.dmc_last_error()
  L.dmc_dist_destroy(None)
  status = ctypes.c_int32(5)
  assert L.dmc_geom_distance_host(7, p, p, p, 2, p, p, p, 1.0, 1e-6, 50, None, ctypes.byref(status)) == 1.0 and status.value == -1
  assert b'mesh' in L.dmc_last_error()
  units = {u[0]: u for u in build._UNITS}
  assert 'dist_core.h' in units['dist_kernels.hip'][2] and not set(units['dist_kernels.hip'][2]) & set(build.STEP_SOURCES) - {'../../include/dmc_model_layout.h'}
  with open(os.path.join(build.CSRC, 'dist_core.h')) as f:
    assert re.findall(r'#include\s+"([^"]+)"', f.read()) == ['../../include/dmc_model_layout.h']      # nothing of the step core
  for src in ('dist_core.h', 'dist_kernels.hip'):
    with open(os.path.join(build.CSRC, src)) as f:
      assert not re.search(r'\basm\b|__asm', f.read())
  # the facade on the CPU oracle: the kinematics as they stand
  monkeypatch.setattr(mj, 'BatchedPhysics', ob.OracleBatch)
  model = mj.MjModel.from_xml_string(dc.xml())
  data = mj.MjData(model)
  for s in (1, 3, 33):
    data.qpos[:] = dc.qpos_of(golden['pos'][s], golden['quat'][s])
    mj.mj_forward(model, data)
    for pi in range(0, 55, 3):
      g1, g2 = dc.PAIRS[pi]
      ft = np.full(6, 7.0)
      d = mj.mj_geomDistance(model, data, g1, g2, dc.DISTMAX, ft)
      ref = min(golden['dist'][s, pi], dc.DISTMAX)
      assert isinstance(d, float) and abs(d - ref) <= dist_bound(64, np.array([ref] * 55))[pi] + 1e-12      # (+ the oracle's poses against the fixture's)
      if golden['unique'][s, pi]:
        assert np.max(np.abs(ft - golden['fromto'][s, pi])) <= dc.WITNESS_TOL[64]
  assert mj.mj_geomDistance(model, data, 1, 2, 0.01, None) == 0.01      # fromto may be None; clipped
  assert mj.mj_geomDistance(model, data, 0, 0, 2.0, None) == 2.0       # plane-plane
  with pytest.raises(mj.FatalError):
    mj.mj_geomDistance(model, data, 0, 99, 1.0, None)


def test_pairs_from_sensors_and_the_compiler_still_refuses_the_elements():
  from dm_control_amd import mjcf_compiler as mc
  sensors = ('<sensor><distance name="d0" geom1="sph0" geom2="box1" cutoff="0.5"/><normal name="n0" body1="b_cap0" geom2="floor"/>'
             '<fromto body1="b_ell0" body2="b_cyl1" cutoff="2"/><touch site="x"/></sensor>')
  got = distance.pairs_from_sensors('<mujoco>%s</mujoco>' % sensors)
  assert got['pairs'] == [('sph0', 'box1'), (dict(body='b_cap0'), 'floor'), (dict(body='b_ell0'), dict(body='b_cyl1'))]
  assert list(got['distmax']) == [0.5, 0.0, 2.0] and got['kinds'] == ['distance', 'normal', 'fromto'] and got['names'] == ['d0', 'n0', None]
  with pytest.raises(ValueError, match='exactly one'):
    distance.pairs_from_sensors('<mujoco><sensor><distance geom1="a" body1="b" geom2="c"/></sensor></mujoco>')
  with pytest.raises(mc.MjcfError, match='unsupported sensor'):
    mc.compile_xml(dc.xml().replace('</worldbody>', '</worldbody>' + sensors.replace('<touch site="x"/>', '')))
  m = mc.compile_xml(dc.xml())
  adr, member, dm = distance.pair_tables(m, got['pairs'], got['distmax'])
  ids = {n: i for i, (n, _, _) in enumerate(dc.GEOMS)}
  assert member.tolist() == [ids['sph0'], ids['box1'], ids['cap0'], ids['floor'], ids['ell0'], ids['cyl1']]
  assert adr.tolist() == [[0, 1, 1, 1], [2, 1, 3, 1], [4, 1, 5, 1]] and dm.tolist() == [0.5, 0.0, 2.0]


def test_members_and_argument_errors_need_no_device():
  from dm_control_amd import mjcf_compiler as mc
  from dm_control_amd.suite import proximity
  m = mc.compile_xml('<mujoco><worldbody><geom name="floor" type="plane" size="1 1 .1"/><body name="arm" pos="0 0 1"><joint/>'
                     '<geom name="u" type="capsule" size=".05 .2"/><geom name="f" type="box" size=".1 .1 .1" pos="0 0 .3"/>'
                     '<body name="bare" pos="0 0 .5"><joint/><inertial pos="0 0 0" mass="1" diaginertia="1 1 1"/></body></body></worldbody></mujoco>')
  assert distance.resolve_member(m, 'u') == [1] and distance.resolve_member(m, 2) == [2] and distance.resolve_member(m, dict(geom='f')) == [2]
  assert distance.resolve_member(m, dict(body='arm')) == [1, 2] and distance.resolve_member(m, dict(body=0)) == [0]
  adr, member, dm = distance.pair_tables(m, [(dict(body='arm'), 'floor'), ('u', 'f')], [1.0, np.inf])
  assert adr.tolist() == [[0, 2, 2, 1], [3, 1, 4, 1]] and member.tolist() == [1, 2, 0, 1, 2] and dm[1] == np.inf
  for bad in (dict(body='bare'), dict(site='x'), 'nogeom', 9, -1, 1.5, dict(body=7)):
    with pytest.raises((ValueError, KeyError)):
      distance.resolve_member(m, bad)
  for pairs, dmax in (([], 1.0), ([('u',)], 1.0), ([('u', 'f')], [1.0, 2.0]), ([('u', 'f')], np.nan)):
    with pytest.raises(ValueError):
      distance.pair_tables(m, pairs, dmax)
  # mesh and height-field members are refused by name; the unit lists them
  fake = types.SimpleNamespace(ngeom=3, nbody=2, geom_type=np.array([6, 7, 1]), geom_bodyid=np.array([0, 1, 1]),
                               names=dict(geom=['crate', 'hull', None]), name2id=lambda n, k: dict(crate=0, hull=1, ship=1)[n])
  assert distance.unsupported_geoms(fake) == ['hull', 2] and distance.resolve_member(fake, 'crate') == [0]
  with pytest.raises(ValueError, match='hull'):
    distance.resolve_member(fake, 'hull')
  with pytest.raises(ValueError, match=r"mesh / height-field.*\['hull', 2\]"):
    distance.resolve_member(fake, dict(body='ship'))
  with pytest.raises(ValueError, match='tolerance'):
    distance.BatchDistance(object(), [('u', 'f')], tolerance=0)
  with pytest.raises(ValueError, match='iterations'):
    distance.BatchDistance(object(), [('u', 'f')], iterations=0)
  with pytest.raises(TypeError, match='BatchedPhysics'):
    distance.BatchDistance(object(), [('u', 'f')])
  with pytest.raises(ValueError, match='scale'):
    proximity.wrap(object(), [('u', 'f')], 1.0, scale='log')
  with pytest.raises(ValueError, match='distmax'):
    proximity.wrap(object(), [('u', 'f')], np.inf, scale='tanh')
  with pytest.raises(ValueError, match='pairs'):
    proximity.wrap(object(), [], 1.0)
  with pytest.raises(TypeError, match='BatchedPhysics'):
    proximity.wrap(object(), [('u', 'f')], 1.0)


def test_sanitized_stand_alone_program_over_the_fixture(tmp_path, golden):
  """csrc/dist_core.h under AddressSanitizer and UBSan: a program with its own main (tests/emu/dist_sanitize.cpp), fed the
  fixture's cases as text, in both precisions -- never through Python, never on a GPU."""
  exe = str(tmp_path / 'dist_sanitize')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                         '-o', exe, os.path.join(ROOT, 'tests', 'emu', 'dist_sanitize.cpp')])
  lines = []
  for s in range(len(golden['pos'])):
    G = dc.geoms_of(golden['pos'][s], golden['quat'][s])
    for p in dc.PAIRS:
      row = []
      for g in (G[p[0]], G[p[1]]):
        row += [repr(int(g.type))] + [repr(float(v)) for v in np.concatenate([g.size, g.pos, g.mat.reshape(9)])]
      lines.append(' '.join(row))
  res = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120, check=False)
  assert res.returncode == 0, res.stderr[-2000:]
  d = np.array([[float(v) for v in l.split()] for l in res.stdout.strip().split('\n')])      # per case: fp64 dist, status, fp32 dist, status
  assert d.shape == (len(lines), 4) and not d[:, 1].any() and not d[:, 3].any()
  ref = np.minimum(golden['dist'], dc.DISTMAX).reshape(-1)
  assert np.all(np.abs(d[:, 0] - ref) <= dist_bound(64, ref.reshape(-1, 55)).reshape(-1))

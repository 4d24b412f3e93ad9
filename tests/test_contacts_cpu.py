"""Contact-level parity of the kernel core's narrow phase with the fp64 oracle, CPU tier: the host build (tests/emu, one
lane per environment) on every case of tests/contact_cases.py.  The gate before tests/test_gpu_contacts.py runs the same
cases on the device; it also keeps the cases themselves honest (contact-rich, within the edge cap, branches reached)."""
import glob
import os

import numpy as np
import pytest

import contact_cases as cc
from dm_control_amd import mjcf_compiler as mc
from emu_lib import EmuPhysics

ALL_PAIRS = cc.PAIRS + cc.GUARDED
_ids = ['%s-%s' % p for p in ALL_PAIRS]
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dm_control_amd', 'suite', 'assets')


def emu_listings(model, qpos, prec, edits=None, **caps):
  out = []
  e = EmuPhysics(model, prec, **caps)
  for k, q in enumerate(qpos):
    if edits is not None:
      e = EmuPhysics(model, prec, **caps)
      edits[k](e)
    e.qpos[:] = q
    e.fi['warning'][:] = 0
    e.forward()
    out.append(cc.Listing(e.ncon[0], e.contact_geom1, e.contact_geom2, e.contact_dist, e.contact_pos, e.contact_frame,
                          np.array(e.warning)))
  return out


@pytest.mark.parametrize('t1,t2', cc.PAIRS, ids=_ids[:len(cc.PAIRS)])
def test_sampler_bears_contacts_of_both_signs_within_the_edge_cap(t1, t2):
  """From the oracle alone: at least half of the sampled poses bear contacts, dist takes both signs, and the edge rule
  leaves out at most EDGE_CAP of them."""
  case = cc.pair_case(t1, t2)
  refs = case.refs[:cc.NPOSE]
  assert sum(r.ncon > 0 for r in refs) >= cc.NPOSE//2
  dist = np.concatenate([r.dist for r in refs])
  assert (dist < 0).any() and (dist > 0).any()
  assert case.edge[:cc.NPOSE].mean() <= cc.EDGE_CAP, case.edge[:cc.NPOSE].mean()


@pytest.mark.parametrize('t1,t2', cc.GUARDED, ids=_ids[len(cc.PAIRS):])
def test_guarded_pairs_never_bear_a_contact_and_warn(t1, t2):
  case = cc.pair_case(t1, t2)
  assert all(r.ncon == 0 for r in case.refs)
  assert sum(r.warning[cc.WARN_COLLISION] > 0 for r in case.refs) >= cc.NPOSE//4
  assert case.edge.mean() <= cc.EDGE_CAP


def test_directed_poses_reach_their_branches():
  """The oracle's own count says that each directed pose is where it was aimed."""
  for name, t1, t2, q, want in cc.directed_poses():
    assert cc.oracle_ref(cc.pair_model(t1, t2), q).ncon == want, name


def test_an_ellipsoid_against_a_box_is_refused_at_create_time():
  with pytest.raises(ValueError, match='not implemented'):
    EmuPhysics(mc.compile_xml(cc.pair_xml(*cc.REFUSED)), 64)


@pytest.mark.parametrize('prec', [64, 32])
@pytest.mark.parametrize('t1,t2', ALL_PAIRS, ids=_ids)
def test_host_build_contacts_match_oracle(t1, t2, prec):
  case = cc.pair_case(t1, t2)
  errs, left_out = cc.check_case(case, emu_listings(case.model, case.qpos, prec, nconmax=8), prec)
  print('%s fp%d: %s, %.3f left out' % (case.name, prec, errs, left_out))
  tol = cc.F64_TOL if prec == 64 else cc.F32_CEILING      # (the measured fp32 bound is the device's: its FMAs differ)
  for k in cc.QUANTITIES:
    assert errs[k] <= tol[case.cls][k], (k, errs[k])


@pytest.mark.parametrize('prec', [64, 32])
def test_host_build_heap_keeps_the_oracles_order_and_its_first_contacts_under_a_cap(prec):
  case = cc.heap_case()
  assert cc.heap_model().nv == 60
  counts = [r.ncon for r in case.refs]
  assert max(counts) <= cc.HEAP_NCONMAX and min(counts) > cc.HEAP_SMALL_CAP
  tol = cc.F64_TOL if prec == 64 else cc.F32_CEILING
  # (njmax = 64: fewer rows than the contacts fill, as the device's fp64 batch at 16 lanes has -- the list is the same)
  for cap, nconmax, njmax in ((None, cc.HEAP_NCONMAX, 0), (None, cc.HEAP_NCONMAX, 64), (cc.HEAP_SMALL_CAP, cc.HEAP_SMALL_CAP, 0)):
    e = EmuPhysics(case.model, prec, nconmax=nconmax, njmax=njmax)
    assert e.nconmax == nconmax and (not njmax or e.njmax == njmax)
    errs, _ = cc.check_case(case, emu_listings(case.model, case.qpos, prec, nconmax=nconmax, njmax=njmax), prec, cap=cap)
    for k in cc.QUANTITIES:
      assert errs[k] <= tol['analytic'][k], (cap, k, errs[k])


# ---- the caps --------------------------------------------------------------------------------------------------------------------
def test_parallel_capsules_keep_both_contacts_when_the_caller_asks_for_room():
  """A model whose candidate pairs are all capsule-capsule: the default caps count one contact per pair (2 only for
  exactly parallel axes), a caller's larger nconmax is admitted up to two per pair, with their rows."""
  m = cc.pair_model('capsule', 'capsule')
  d = EmuPhysics(m, 64)
  assert (d.nconmax, d.njmax) == (1, 4)
  e = EmuPhysics(m, 64, nconmax=8)
  assert (e.nconmax, e.njmax) == (2, 8)
  q = [p for n, _, _, p, _ in cc.directed_poses() if n == 'parallel capsules'][0]
  ref = cc.oracle_ref(m, q)
  for prec in (64, 32):
    got = emu_listings(m, [q], prec, nconmax=8)[0]
    assert got.ncon == ref.ncon == 2 and not got.warning.any()
    # the default cap drops the second contact and says so
    got = emu_listings(m, [q], prec)[0]
    assert got.ncon == 1 and got.warning[cc.WARN_CONTACTFULL] == 1


def test_suite_assets_keep_their_caps():
  """The baked layouts, tests/test_lds_budget.py and the benchmark's shapes depend on the caps of the suite models."""
  from dm_control_amd.suite import common
  assert sorted(cc.SUITE_CAPS) == sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(ASSETS, '*.xml')))
  for name, (asked, nconmax, njmax) in cc.SUITE_CAPS.items():
    assert common.DEFAULT_CAPS.get(name, {}).get('nconmax', 0) == asked, name
    with open(os.path.join(ASSETS, name + '.xml')) as f:
      e = EmuPhysics(mc.compile_xml(f.read()), 64, nconmax=asked)
    assert (e.nconmax, e.njmax) == (nconmax, njmax), name

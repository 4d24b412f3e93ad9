"""Host-derived mjData arrays of this tree against those of another revision, on the fp64 oracle stand-in (no GPU).

  python scripts/host_data_parity.py --parent HEAD [--out profiles/host_data_parity.json]

extracts `--parent` with `git archive` into a temporary directory, dumps the quantities below from that checkout and from
this tree (one child process each: `--dump FILE --root DIR`), and writes the per-quantity maximum absolute difference.
Models: cheetah, humanoid, quadruped, the ball chain of tests/test_mujoco_api.py, the tendon model of
tests/test_facade_cpu.py.  Through `mujoco_api.MjData`: xanchor xaxis ten_length ten_velocity wrap_xpos, the four object
velocities (world and local frame), mj_getState for three signatures, M qLD subtree_linvel subtree_angmom act_dot
qfrc_passive.  Through `physics.Physics` at B = 2 (two different states): xanchor xaxis ten_length ten_velocity, the object
velocities, get_state for the same signatures.

Code that only moved must come out bit-equal; a quantity whose formula changed form may differ by the tolerance at which
the tests already compare it with the oracle (BOUNDS); anything else makes the script fail.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = (0b1110, (1 << 13) - 1, 1 | 16 | 32 | 64 | 512)      # mjSTATE_PHYSICS, every bit, time | warmstart | ctrl | qfrc_applied | mocap_pos


# quantity (by the last part of its key) -> the tolerance the tests compare it with the oracle at; everything else: 0
BOUNDS = (('xanchor', 1e-14), ('xaxis', 1e-14), ('ten_length', 1e-12), ('ten_velocity', 1e-12), ('wrap_xpos', 1e-12),
          ('object_velocity', 1e-6))


def facades(root):
  """(mujoco_api, physics, {model name: xml}) of the checkout at `root`, both facades on the oracle stand-in."""
  sys.path[:0] = [root, os.path.join(root, 'tests')]
  import oracle_backend
  from dm_control_amd import mujoco_api as mj
  from dm_control_amd import physics
  from dm_control_amd.suite import common
  from test_facade_cpu import _TENDON_XML
  from test_mujoco_api import _BALL_CHAIN
  mj.BatchedPhysics = physics.BatchedPhysics = oracle_backend.OracleBatch
  models = {n: common.read_model(n + '.xml') for n in ('cheetah', 'humanoid', 'quadruped')}
  models.update(ball_chain=_BALL_CHAIN, tendons=_TENDON_XML)
  return mj, physics, models


def shaken(mj, xml, seed):
  """(MjModel, MjData) a few steps after a random state, forwarded."""
  m = mj.MjModel.from_xml_string(xml)
  d = mj.MjData(m)
  c, rs = m._c, np.random.RandomState(seed)
  d.qpos[:] = c.qpos0 + rs.uniform(-.3, .3, c.nq)
  for j in range(c.njnt):
    if c.jnt_type[j] in (0, 1):
      a = int(c.jnt_qposadr[j]) + (3 if c.jnt_type[j] == 0 else 0)
      q = rs.normal(size=4)
      d.qpos[a:a + 4] = q / np.linalg.norm(q)
  d.qvel[:] = rs.uniform(-1, 1, c.nv)
  d.ctrl[:] = rs.uniform(-1, 1, c.nu)
  mj.mj_step(m, d, 7)
  mj.mj_forward(m, d)
  return m, d


def objects(c):
  out = [('body', 1, c.nbody - 1), ('xbody', 2, c.nbody - 1), ('geom', 5, c.ngeom - 1)]
  return out + ([('site', 6, c.nsite - 1)] if c.nsite else [])


def dump(root, path):
  mj, physics, models = facades(root)
  out = {}
  for name, xml in models.items():
    pairs = [shaken(mj, xml, seed) for seed in (0, 1)]
    m, d = pairs[0]
    c = m._c
    for f in ('xanchor', 'xaxis', 'ten_length', 'ten_velocity', 'wrap_xpos', 'M', 'qLD', 'act_dot', 'qfrc_passive'):
      try:
        out['%s/mjdata/%s' % (name, f)] = np.array(getattr(d, f))
      except NotImplementedError:      # (qfrc_passive of a model with fluid forces)
        pass
    d.subtree_linvel, d.subtree_angmom      # pylint: disable=pointless-statement  (handed out: mj_subtreeVel fills them)
    mj.mj_subtreeVel(m, d)
    out[name + '/mjdata/subtree_linvel'], out[name + '/mjdata/subtree_angmom'] = d.subtree_linvel.copy(), d.subtree_angmom.copy()
    for kind, objtype, objid in objects(c):
      for local in (0, 1):
        res = np.zeros(6)
        mj.mj_objectVelocity(m, d, objtype, objid, res, local)
        out['%s/mjdata/object_velocity_%s_%d' % (name, kind, local)] = res
    for sig in SIGS:
      state = np.zeros(mj.mj_stateSize(m, sig))
      mj.mj_getState(m, d, state, sig)
      out['%s/mjdata/state_%d' % (name, sig)] = state
    p = physics.Physics(physics.mjcf_compiler.compile_xml(xml), batch_size=2)
    with p.reset_context():
      for f in ('qpos', 'qvel', 'act', 'ctrl'):
        if getattr(d, f).size:
          setattr(p.data, f, np.stack([np.array(getattr(dd, f)) for _, dd in pairs]))
    for f in ('xanchor', 'xaxis') + (('ten_length', 'ten_velocity') if c.ntendon else ()):
      out['%s/physics/%s' % (name, f)] = np.array(getattr(p.data, f))
    for kind, _, objid in objects(c):
      for local in (0, 1):
        out['%s/physics/object_velocity_%s_%d' % (name, kind, local)] = p.data.object_velocity(objid, kind, local_frame=bool(local))
    for sig in SIGS:
      out['%s/physics/state_%d' % (name, sig)] = p.get_state(sig)
    p.free()
  np.savez(path, **out)


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--parent', help='the revision to compare with')
  ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'host_data_parity.json'))
  ap.add_argument('--dump', help='(child) write the quantities of the checkout at --root to this .npz')
  ap.add_argument('--root', default=HERE)
  args = ap.parse_args()
  if args.dump:
    return dump(args.root, args.dump)
  with tempfile.TemporaryDirectory() as tmp:
    parent = os.path.join(tmp, 'parent')
    os.mkdir(parent)
    tar = subprocess.run(['git', '-C', HERE, 'archive', args.parent], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(['tar', '-x', '-C', parent], input=tar, check=True)
    got = {}
    for tag, root in (('parent', parent), ('tree', HERE)):
      path = os.path.join(tmp, tag + '.npz')
      subprocess.run([sys.executable, os.path.abspath(__file__), '--dump', path, '--root', root], check=True, cwd=root)
      got[tag] = dict(np.load(path))
  if set(got['parent']) != set(got['tree']):
    raise SystemExit('the two revisions serve different quantities: %s' % sorted(set(got['parent']) ^ set(got['tree'])))
  diff = {}
  for k in sorted(got['tree']):
    a, b = got['parent'][k], got['tree'][k]
    if a.shape != b.shape:
      raise SystemExit('%s: shape %s became %s' % (k, a.shape, b.shape))
    diff[k] = float(np.abs(a - b).max(initial=0.0))
  rev = subprocess.run(['git', '-C', HERE, 'rev-parse', args.parent], check=True, stdout=subprocess.PIPE, text=True).stdout.strip()
  bound = lambda k: next((tol for name, tol in BOUNDS if k.split('/')[-1].startswith(name)), 0.0)
  over = {k: v for k, v in diff.items() if v > bound(k)}
  result = {'parent': rev, 'device': 'fp64 oracle stand-in (tests/oracle_backend.py)', 'quantities': len(diff),
            'bit_equal': sum(v == 0.0 for v in diff.values()), 'bounds': dict(BOUNDS),
            'not_bit_equal': {k: v for k, v in diff.items() if v != 0.0}, 'over_bound': over, 'max_abs_diff': diff}
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write('\n')
  print(json.dumps({k: result[k] for k in ('quantities', 'bit_equal', 'not_bit_equal', 'over_bound')}, indent=1))
  if over:
    raise SystemExit('differences beyond the bound: %s' % sorted(over))


if __name__ == '__main__':
  main()

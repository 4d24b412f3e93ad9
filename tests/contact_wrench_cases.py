"""TEST INFRASTRUCTURE: the shared cases of the contact-wrench unit's tests (tests/test_contact_wrench_cpu.py,
tests/test_gpu_contact_wrench.py).

Fixture (a): a free box on a plane (BOX_XML).  Fixture (b): a "biped" -- a torso on a free joint, two legs of thigh, shin
and box foot, a loose ball -- on a plane, compiled with pyramidal and with elliptic cones.  Only the floor, the two feet
and the ball collide (the torso and the leg capsules have contype = conaffinity = 0), so the collidable pairs are few and
every one of them has a closed-form distance or a bounding-sphere bound.  The ball has condim 6 (its contacts carry a
torque: t_c != 0), the floor and the right foot condim 1 (their pair takes the one-row path), the left foot condim 3.
Every geom has margin 0.01 and soft contacts (solref 0.05): a resting contact settles 6 to 8 mm inside the margin instead
of hovering at it.  An accelerometer makes the oracle run rne_post_constraint and expose cfrc_ext.

The 16 states are short oracle roll-outs from seeded starts (`start`): the biped standing with bent legs near its resting
height, with both feet on the floor, with one foot lifted clear of the margin, or (states 0 and 8) still in the air; the
ball in the air, on the floor far from the feet, on the left foot, or moving against the outer side of the left foot while
it lies on the floor -- there the ball's geom is geom2 of the floor's contact and geom1 of the foot's, so a ball target
counts contacts with both signs.  What the tests rely on is ASSERTED by `check_states`, not trusted: a state with
ncon == 0, a state with ncon == the largest, differing ncon, both signs, condim 1, 3 and 6 contacts with t_c != 0, and every
collidable pair at least MARGIN_CLEARANCE away from the margin, so that no precision gains or loses a contact.

References, none of them the code under test: tests/con_twin.py on a contact list (R1), the oracle's cfrc_ext (R2), the
box's weight (R3), Newton's third law (R4).
"""
import numpy as np

from dm_control_amd import contacts      # noqa: F401  (the unit these cases belong to: without it they are not importable)
from dm_control_amd import mjcf_compiler

import con_twin
import dist_twin

NSTATE = 16
SEED = 2031
MARGIN = 0.01
MARGIN_CLEARANCE = 1e-3
REST = 0.002            # about where a resting contact of the soft (solref 0.05) geoms settles: 8 mm inside the margin
B_GPU = 70              # environment e holds state e % NSTATE
F64_TOL = 1e-9          # x max(1, |reference|max): the project's bar for its fp64 units
# fp32: the worst error of the fp32 HOST build of csrc/con_core.h on fp32-rounded inputs against the fp64 twin over both cones,
# every state and every target of TARGETS (measured and printed by
# test_contact_wrench_cpu.py::test_fp32_host_build_against_the_fp64_twin), relative to max(1, |reference|max) per output.
# The bound is 4 x the measured value, on the CPU and on the GPU.
# (wrench is small because the fixture's contact frames are nearly axis-aligned: their products round little; dist is a
# minimum of the inputs and exact)
F32_MEASURED = dict(wrench=3.42e-9, force=1.53e-7, torque=9.66e-8, normal=8.52e-8, dist=0.0)
F32_TOL = {k: 4 * v for k, v in F32_MEASURED.items()}
# End to end on the device after forward() at the uploaded states, against the oracle (R1 on its contact list, R2): the
# parity of the device's SOLVER, not of this unit.  Measured by test_gpu_contact_wrench.py::test_end_to_end_against_the_oracle,
# relative to max(1, |reference|max) per output (cfrc_*: whole-body targets against the oracle's cfrc_ext); the bound is 4 x
# the measured value.
E2E_MEASURED = {64: dict(force=2.18e-14, torque=2.76e-14, normal=2.18e-14, dist=2.26e-16, cfrc_force=2.72e-14, cfrc_torque=2.59e-14),
                32: dict(force=5.48e-6, torque=4.79e-6, normal=5.48e-6, dist=1.84e-7, cfrc_force=6.23e-6, cfrc_torque=6.07e-6)}
# R3: the resting box's normal force against m g.  The solver stops at a relative tolerance of 1e-8, so the fp64 residual
# of M qacc = qfrc + J'f is of that order: 100 x that for fp64; fp32 holds the project's fp32 bar (1e-4, as in smoke()).
WEIGHT_TOL = {64: 1e-6, 32: 1e-4}
OUTPUTS = ('force', 'torque', 'normal', 'count', 'dist')

BOX_MASS, BOX_XML = 2.0, """<mujoco model="box_on_plane">
  <option timestep="0.005"/>
  <worldbody>
    <geom name="floor" type="plane" size="2 2 .1" margin="0.01"/>
    <body name="box" pos="0 0 .0495">
      <joint name="box_root" type="free"/>
      <geom name="box" type="box" size=".05 .05 .05" mass="2" margin="0.01"/>
    </body>
  </worldbody>
</mujoco>"""

_LEG = """
      <body name="thigh_{s}" pos="0 {y} -.1">
        <joint name="hip_{s}" type="hinge" axis="0 1 0"/>
        <geom name="thigh_{s}" type="capsule" fromto="0 0 0 0 0 -.2" size=".03" contype="0" conaffinity="0" mass="1.5"/>
        <body name="shin_{s}" pos="0 0 -.2">
          <joint name="knee_{s}" type="hinge" axis="0 1 0"/>
          <geom name="shin_{s}" type="capsule" fromto="0 0 0 0 0 -.2" size=".025" contype="0" conaffinity="0" mass="1"/>
          <body name="foot_{s}" pos="0 0 -.23">
            <joint name="ankle_{s}" type="hinge" axis="0 1 0"/>
            <geom name="foot_{s}" type="box" size=".09 .04 .02" pos=".03 0 0" condim="{condim}" mass=".5"/>
          </body>
        </body>
      </body>"""


def biped_xml(cone='pyramidal'):
  return """<mujoco model="biped">
  <option timestep="0.005" cone="%s"/>
  <default><geom margin="0.01" solref="0.05 1"/><joint damping="5" armature="0.01"/></default>
  <worldbody>
    <geom name="floor" type="plane" size="4 4 .1" condim="1"/>
    <body name="ball" pos=".6 0 .04">
      <joint name="ball_root" type="free" damping="0" armature="0"/>
      <geom name="ball" type="sphere" size=".04" condim="6" friction="1 .01 .001" mass=".3"/>
    </body>
    <body name="torso" pos="0 0 .55">
      <joint name="root" type="free" damping="0" armature="0"/>
      <geom name="torso" type="box" size=".06 .12 .1" contype="0" conaffinity="0" mass="6"/>
      <site name="imu" pos="0 0 .05"/>%s%s
    </body>
  </worldbody>
  <sensor><accelerometer name="acc" site="imu"/></sensor>
</mujoco>""" % (cone, _LEG.format(s='l', y='.1', condim=3), _LEG.format(s='r', y='-.1', condim=1))


CONES = ('pyramidal', 'elliptic')
_models, _states, _refs = {}, {}, {}


def model(cone='pyramidal'):
  if cone not in _models:
    _models[cone] = mjcf_compiler.compile_xml(BOX_XML if cone == 'box' else biped_xml(cone))
  return _models[cone]


# every form of a target: geom, body, subtree, with and without `other`, overlapping
TARGETS = ['foot_l', dict(geom='foot_r'), dict(body='foot_l', other='floor'), dict(body='foot_r', other='floor'),
           dict(body='ball'), dict(body='ball', other=dict(body='thigh_l', subtree=True)), dict(body='torso', subtree=True),
           dict(body='thigh_l', subtree=True), dict(body='thigh_r', subtree=True, other=dict(geom='floor')),
           dict(geom='floor'), dict(geom=['foot_l', 'foot_r']), dict(body='foot_l', other='ball'),
           dict(geom='floor', other=dict(body='torso', subtree=True)), dict(body='torso'), dict(body='world')]
# whole bodies with `other` unset: what the oracle's cfrc_ext holds (R2); (target, body name)
BODY_TARGETS = [(dict(body=b), b) for b in ('ball', 'torso', 'thigh_l', 'shin_l', 'foot_l', 'thigh_r', 'shin_r', 'foot_r')]


def targets64(m):
  """T = 64: the targets of TARGETS repeated, and every geom on its own."""
  t = list(TARGETS) + [dict(geom=g) for g in range(m.ngeom)]
  return (t * (64 // len(t) + 1))[:64]


def start(m, s, rs):
  """The seeded start of state `s`: (qpos, qvel, steps of the roll-out)."""
  q, v = np.array(m.qpos0, dtype=np.float64), rs.uniform(-0.02, 0.02, m.nv)
  adr = lambda j: int(m.jnt_qposadr[m.name2id(j, 'joint')])
  dof = lambda j: int(m.jnt_dofadr[m.name2id(j, 'joint')])
  ball, root = adr('ball_root'), adr('root')
  # bent legs with the feet kept flat (hip -b, knee 2b, ankle -b); a leg bent by b lifts its foot by 0.43 (1 - cos b).
  # One leg bent far more than the other leaves that foot in the air, well outside the margin.
  both = rs.uniform(0.0, 0.2)
  bend = dict(l=0.3 if s in (12, 13) else both, r=0.3 if s in (4, 5, 6, 7) else both)
  if s in (4, 5, 6, 7, 12, 13):
    bend['r' if bend['l'] == 0.3 else 'l'] = 0.0
  for side, b in bend.items():
    q[adr('hip_' + side)], q[adr('knee_' + side)], q[adr('ankle_' + side)] = -b, 2*b, -b
  hover = lambda: REST + rs.uniform(0.0, 0.002)      # a contact distance near the resting one: REST below the margin's reach
  lift = hover()
  q[root + 2] += lift - 0.43*(1 - np.cos(min(bend.values()))) + (0.3 if s in (0, 8) else 0.0)      # (0, 8): still in the air
  mode = s % 4
  if mode == 0:      # the ball in the air
    q[ball:ball + 3] = [0.6, 0.3, 0.5]
  elif mode == 1:    # on the floor, far from the feet
    q[ball:ball + 3] = [0.6 + rs.uniform(-.05, .05), rs.uniform(-.2, .2), 0.04 + hover()]
  elif mode == 2:    # on the left foot
    q[ball:ball + 3] = [0.06 + rs.uniform(-.01, .01), 0.1 + rs.uniform(-.005, .005), 0.04 + lift + 0.04 + hover()]
  else:              # pressed against the outer side of the left foot while it lies on the floor
    q[ball:ball + 3] = [0.03 + rs.uniform(-.02, .02), 0.1 + 0.04 + 0.04 + 0.005, 0.04 + hover()]
    v[dof('ball_root') + 1] = -0.3
  return q, v, (3 if s in (0, 8) else 2 + s % 3)


def states(cone='pyramidal'):
  """(qpos (16, nq), qvel (16, nv)) of the fixture: oracle roll-outs of the seeded starts."""
  if cone not in _states:
    from oracle.oracle import OraclePhysics      # pylint: disable=import-outside-toplevel
    m = model(cone)
    rs = np.random.RandomState(SEED)
    qs, vs = [], []
    for s in range(NSTATE):
      q, v, nstep = start(m, s, rs)
      p = OraclePhysics(m)
      p.qpos[:] = q
      p.qvel[:] = v
      p.forward()
      p.step(nstep)
      qs.append(np.array(p.qpos))
      vs.append(np.array(p.qvel))
    _states[cone] = (np.array(qs), np.array(vs))
  return _states[cone]


def oracle_state(m, qpos, qvel):
  """The oracle after forward() at a state: dict(contacts (con_twin's list, with dim and efc_address), ncon, xpos, xipos,
  xmat, subtree_com, cfrc_ext (nbody, 6) (torque, force), qacc, geom_xpos, geom_xmat)."""
  from oracle.oracle import OraclePhysics      # pylint: disable=import-outside-toplevel
  p = OraclePhysics(m)
  p.qpos[:] = qpos
  p.qvel[:] = qvel
  p.forward()
  g = lambda n, *s: np.array(p.field(n), dtype=np.float64).reshape(*s)
  cons = []
  for i in range(int(p.ncon)):
    c = p.contact(i)
    cons.append(dict(geom1=c['geom1'], geom2=c['geom2'], dist=float(c['dist']), pos=np.array(c['pos']), frame=np.array(c['frame']),
                     force=np.array(p.contact_force(i)).reshape(6), dim=c['dim'], efc_address=c['efc_address']))
  assert not np.asarray(p.warning).any(), 'the oracle raised a warning'
  return dict(contacts=cons, ncon=len(cons), xpos=g('xpos', -1, 3), xipos=g('xipos', -1, 3), xmat=g('xmat', -1, 3, 3),
              subtree_com=g('subtree_com', -1, 3), cfrc_ext=g('cfrc_ext', -1, 6), qacc=g('qacc', -1),
              geom_xpos=g('geom_xpos', -1, 3), geom_xmat=g('geom_xmat', -1, 3, 3))


def references(cone='pyramidal'):
  """[oracle_state] of the 16 states, computed once."""
  if cone not in _refs:
    m = model(cone)
    q, v = states(cone)
    _refs[cone] = [oracle_state(m, q[s], v[s]) for s in range(NSTATE)]
  return _refs[cone]


def nconmax(cone='pyramidal'):
  return max(r['ncon'] for r in references(cone))


def arrays(refs, K):
  """The unit's input arrays, environment-major, of a list of oracle states (con_emu_lib.FIELDS); slots past ncon hold
  geom ids of -1 and zeros, as the step kernels leave them."""
  B = len(refs)
  a = dict(ncon=np.zeros(B, np.int32), geom1=np.full((B, K), -1, np.int32), geom2=np.full((B, K), -1, np.int32), dist=np.zeros((B, K)),
           pos=np.zeros((B, K, 3)), frame=np.zeros((B, K, 3, 3)), force=np.zeros((B, K, 6)))
  for e, r in enumerate(refs):
    a['ncon'][e] = r['ncon']
    for i, c in enumerate(r['contacts']):
      a['geom1'][e, i], a['geom2'][e, i], a['dist'][e, i] = c['geom1'], c['geom2'], c['dist']
      a['pos'][e, i], a['frame'][e, i], a['force'][e, i] = c['pos'], c['frame'], c['force']
  for k in ('xpos', 'xipos', 'xmat'):
    a[k] = np.stack([r[k] for r in refs])
  return a


def contact_list(a, e):
  """Environment e of `arrays`-shaped data (from the oracle or read back from a device) as con_twin's list."""
  return [dict(geom1=int(a['geom1'][e, i]), geom2=int(a['geom2'][e, i]), dist=float(a['dist'][e, i]), pos=np.asarray(a['pos'][e, i]),
               frame=np.asarray(a['frame'][e, i]).reshape(3, 3), force=np.asarray(a['force'][e, i]).reshape(6))
          for i in range(int(a['ncon'][e]))]


def twin_sets(m, target):
  """(S, O | None, named body) of a target as Python sets, resolved HERE from the model's names and tree -- not with
  host_data.contact_targets."""
  names = m.names
  parent = [int(x) for x in m.body_parentid]
  gbody = [int(x) for x in np.asarray(m.geom_bodyid).reshape(-1)]

  def one(spec):
    if not isinstance(spec, dict):
      spec = dict(geom=spec)
    if 'geom' in spec:
      keys = spec['geom'] if isinstance(spec['geom'], (list, tuple)) else [spec['geom']]
      ids = [names['geom'].index(k) if isinstance(k, str) else int(k) for k in keys]
      return set(ids), gbody[ids[0]]
    b = names['body'].index(spec['body']) if isinstance(spec['body'], str) else int(spec['body'])
    bodies = {b}
    if spec.get('subtree'):
      for x in range(m.nbody):
        a = x
        while a != 0 and a != b:
          a = parent[a]
        if a == b:
          bodies.add(x)
    return {g for g in range(m.ngeom) if gbody[g] in bodies}, b

  other = target.get('other') if isinstance(target, dict) else None
  S, body = one({k: v for k, v in target.items() if k != 'other'} if isinstance(target, dict) else target)
  return S, (None if other is None else one(other)[0]), body


def twin_net(m, a, e, target, about='com', local=False):
  """con_twin.net for environment e of `arrays`-shaped data."""
  S, O, body = twin_sets(m, target)
  r = np.zeros(3) if about == 'world' else np.asarray(a['xipos' if about == 'com' else 'xpos'][e]).reshape(-1, 3)[body]
  R = np.asarray(a['xmat'][e]).reshape(-1, 3, 3)[body] if local else None
  return con_twin.net(contact_list(a, e), dict(S=S, O=O, r=r, R=R))


def twin_all(m, a, targets, about='com', local=False):
  """dict(force, torque (B, T, 3), normal, dist (B, T), count (B, T), wrench (B, K, 6)) of the twin over every environment."""
  B, K, T = len(a['ncon']), a['geom1'].shape[1], len(targets)
  out = dict(force=np.zeros((B, T, 3)), torque=np.zeros((B, T, 3)), normal=np.zeros((B, T)), dist=np.zeros((B, T)),
             count=np.zeros((B, T), np.int32), wrench=np.zeros((B, K, 6)))
  for e in range(B):
    out['wrench'][e] = con_twin.wrench(contact_list(a, e), K)
    for t, tg in enumerate(targets):
      r = twin_net(m, a, e, tg, about, local)
      for k in OUTPUTS:
        out[k][e, t] = r[k]
  return out


def rel_error(got, ref):
  """|got - ref|max relative to max(1, |ref|max); +inf entries must agree exactly and are left out of the norm."""
  got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
  inf = np.isinf(ref)
  assert np.array_equal(inf, np.isinf(got)) and np.array_equal(got[inf], ref[inf])
  if inf.all():
    return 0.0
  return float(np.abs(got[~inf] - ref[~inf]).max() / max(1.0, np.abs(ref[~inf]).max()))


def round32(a):
  return {k: (v if v.dtype.kind == 'i' else v.astype(np.float32).astype(np.float64)) for k, v in a.items()}


def cfrc_reference(m, ref, body, about='com'):
  """(force, torque about r) of the contacts on a whole body from the oracle's cfrc_ext (R2): cfrc_ext is (torque about the
  root's subtree_com, force); the torque moves to r by  t_r = t_com + (com - r) x f."""
  b = m.name2id(body, 'body')
  t, f = ref['cfrc_ext'][b, :3], ref['cfrc_ext'][b, 3:]
  com = ref['subtree_com'][int(m.body_rootid[b])]
  r = np.zeros(3) if about == 'world' else ref['xipos' if about == 'com' else 'xpos'][b]
  return f.copy(), t + np.cross(com - r, f)


def pair_clearances(m, ref):
  """|distance - margin| of everything that could become or cease to be a contact in this state: every detected contact
  (from the oracle's list), every corner of a box against the plane that is not one, every other collidable pair from its
  closed form or tests/dist_twin.py -- or a bounding-sphere bound where that already shows the pair far away."""
  out = []
  for c in ref['contacts']:
    out.append(('contact', c['geom1'], c['geom2'], abs(c['dist'] - MARGIN)))
  detected = {(c['geom1'], c['geom2']) for c in ref['contacts']}
  for g1, g2 in zip(m.pair_geom1, m.pair_geom2):
    g1, g2 = int(g1), int(g2)
    t1, t2 = int(m.geom_type[g1]), int(m.geom_type[g2])
    p1, p2, R1, R2 = ref['geom_xpos'][g1], ref['geom_xpos'][g2], ref['geom_xmat'][g1], ref['geom_xmat'][g2]
    if t1 == dist_twin.PLANE and t2 == dist_twin.BOX:      # every corner is a contact of its own
      n, s = R1[:, 2], np.asarray(m.geom_size[g2])
      for sx in (-1, 1):
        for sy in (-1, 1):
          for sz in (-1, 1):
            d = float(n @ (p2 + R2 @ (s * np.array([sx, sy, sz])) - p1))
            out.append(('corner', g1, g2, abs(d - MARGIN)))
      continue
    if (g1, g2) in detected:
      continue      # a single-contact pair: its contact is in the list
    if t1 == dist_twin.PLANE:
      d = dist_twin.plane_distance(dist_twin.Geom(t1, m.geom_size[g1], p1, R1), dist_twin.Geom(t2, m.geom_size[g2], p2, R2))[0]
    else:
      lower = float(np.linalg.norm(p2 - p1) - m.geom_rbound[g1] - m.geom_rbound[g2])      # the bounding spheres' gap: dist >= lower
      if lower - MARGIN >= MARGIN_CLEARANCE:
        out.append(('bound', g1, g2, lower - MARGIN))
        continue
      d = dist_twin.distance(dist_twin.Geom(t1, m.geom_size[g1], p1, R1), dist_twin.Geom(t2, m.geom_size[g2], p2, R2))['dist']
    out.append(('pair', g1, g2, abs(d - MARGIN)))
  return out


def check_states(cone):
  """Asserts what the tests rely on (module docstring); returns a summary."""
  m, refs = model(cone), references(cone)
  ncon = [r['ncon'] for r in refs]
  K = max(ncon)
  assert min(ncon) == 0 and ncon.count(K) >= 1 and len(set(ncon)) >= 4, ncon
  assert all(float(m.geom_margin[g]) == MARGIN for g in range(m.ngeom))
  worst = min(c[3] for r in refs for c in pair_clearances(m, r))
  assert worst >= MARGIN_CLEARANCE, worst
  a = arrays(refs, K)
  S, _, _ = twin_sets(m, dict(body='ball'))
  signs = [set(con_twin.net(contact_list(a, e), dict(S=S, O=None, r=np.zeros(3)))['signs']) for e in range(NSTATE)]
  assert any({1, -1} <= s for s in signs), signs      # the ball is geom2 of the floor's contact and geom1 of the foot's
  dims = {c['dim'] for r in refs for c in r['contacts']}
  assert {1, 3, 6} <= dims, dims
  spin = max(np.abs(con_twin.world_wrench(c)[1]).max() for r in refs for c in r['contacts'] if c['dim'] == 6)
  assert spin > 1e-6, spin      # t_c != 0 somewhere
  assert all(c['efc_address'] >= 0 for r in refs for c in r['contacts'])      # every contact is in the constraint set
  multi = max(twin_net(m, a, e, dict(body='foot_l'))['count'] for e in range(NSTATE))
  assert multi >= 4, multi      # a box foot gives several contacts per target
  return dict(ncon=ncon, nconmax=K, clearance=worst, dims=sorted(dims), spin=spin)

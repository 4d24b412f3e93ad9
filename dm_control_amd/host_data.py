"""What the two host facades (`physics.Physics` / `_Data` and `mujoco_api.MjModel` / `MjData`) share: the mjData arrays the
fused kernel never stores, derived from the device's kinematics, and MuJoCo's state layout.

numpy only, no facade state, every function pure: `c` is a compiled `mjcf_compiler.Model`, everything else arrives as
arrays (or as a `get(name, *shape)` reader of them).  The functions both facades call (`joint_frames`, `tendons`,
`object_velocity`, the row helpers) take arbitrary leading batch axes -- `(..., n, 3)` is one environment or `B` of them,
and the batched result equals the per-environment ones to the bit.  The derivations only `MjData` serves (`mass_matrix`, `rne`,
`passive`, `act_dot`, `subtree_vel`) take one environment.

This module never imports `BatchedPhysics`: tests swap that name in each facade separately, so `create_batch` takes the
class from its caller.
"""
import numpy as np

from dm_control_amd import mjcf_compiler

C = mjcf_compiler.C
MINVAL = C['DMC_MINVAL']

# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------
# the mjData arrays a caller writes and the next launch reads (`time` is an input too: each facade handles it itself)
INPUT_FIELDS = ('qpos', 'qvel', 'act', 'ctrl', 'qacc_warmstart', 'qfrc_applied', 'xfrc_applied', 'mocap_pos', 'mocap_quat')
# model arrays tasks may rewrite between episodes; changes are pushed to the device tables in place before the next launch
MUTABLE_MODEL_FIELDS = ('dof_damping', 'jnt_stiffness', 'jnt_range', 'jnt_margin', 'qpos_spring', 'site_pos', 'site_quat',
                        'site_size', 'actuator_ctrlrange', 'actuator_forcerange', 'wrap_prm', 'body_pos', 'body_quat',
                        # geom frames / sizes as tasks rewrite them (suite/reacher.py:88-94, suite/fish.py:150-154: the
                        # target geom); like MuJoCo, nothing derived at compile time (inertias, geom_rbound) follows
                        'geom_pos', 'geom_quat', 'geom_size')
# contact capacities tried, in order, when the caller names none: MuJoCo sizes its contact buffer from an arena (any
# number of contacts a model can produce fits), a drop-in user never sets `nconmax` -- so the facades ask for a generous
# cap first and settle for less only where the model's scratch would not fit in LDS.  (The throughput path,
# BatchedPhysics / suite.load, keeps its tuned per-model caps: suite/common.py DEFAULT_CAPS.)
AUTO_NCONMAX = (64, 48, 32, 0)
# mjtState bits (mujoco 3.x) in the order mj_getState concatenates them: (mjSTATE_<name>, mjData field)
STATE_FIELDS = (('TIME', 'time'), ('QPOS', 'qpos'), ('QVEL', 'qvel'), ('ACT', 'act'), ('WARMSTART', 'qacc_warmstart'),
                ('CTRL', 'ctrl'), ('QFRC_APPLIED', 'qfrc_applied'), ('XFRC_APPLIED', 'xfrc_applied'),
                ('EQ_ACTIVE', 'eq_active'), ('MOCAP_POS', 'mocap_pos'), ('MOCAP_QUAT', 'mocap_quat'), ('USERDATA', None),
                ('PLUGIN', None))
NSTATE = len(STATE_FIELDS)
# qpos / qvel entries per joint type (free, ball, slide, hinge)
JNT_NQ = {0: 7, 1: 4, 2: 1, 3: 1}
JNT_NV = {0: 6, 1: 3, 2: 1, 3: 1}
# mj_objectVelocity's object kinds, by name and by mjtObj: (name table, position field, orientation field | None: the
# inertial frame of a body, xquat * body_iquat)
OBJECT_KINDS = {'body': ('body', 'xipos', None), 'xbody': ('body', 'xpos', 'xmat'), 'geom': ('geom', 'geom_xpos', 'geom_xmat'),
                'site': ('site', 'site_xpos', 'site_xmat')}
OBJECT_KINDS.update({C['DMC_OBJ_' + k.upper()]: v for k, v in list(OBJECT_KINDS.items())})


def state_parts(c, sig):
  """[(mjSTATE name, mjData field | None, size)] of the components `sig` selects, in bit order.  (The callers check `sig`:
  each raises its own error type.)"""
  nm = int(getattr(c, 'nmocap', 0))
  sizes = {'TIME': 1, 'QPOS': c.nq, 'QVEL': c.nv, 'ACT': c.na, 'WARMSTART': c.nv, 'CTRL': c.nu, 'QFRC_APPLIED': c.nv,
           'XFRC_APPLIED': 6 * c.nbody, 'EQ_ACTIVE': len(getattr(c, 'eq_active0', ())), 'MOCAP_POS': 3 * nm,
           'MOCAP_QUAT': 4 * nm, 'USERDATA': 0, 'PLUGIN': 0}      # (no user data / plugins in a compiled Model)
  return [(n, f, int(sizes[n])) for i, (n, f) in enumerate(STATE_FIELDS) if int(sig) & (1 << i)]


def joint_spans(c):
  """(first qpos entry, qpos entries, first dof, dofs) per joint."""
  return (c.jnt_qposadr, [JNT_NQ[int(t)] for t in c.jnt_type], c.jnt_dofadr, [JNT_NV[int(t)] for t in c.jnt_type])


# ---------------------------------------------------------------------------------------------------------------------
# the batch: contact capacity fallback, the xfrc_applied rule, contact records
# ---------------------------------------------------------------------------------------------------------------------
def create_batch(factory, model, batch_size, **kw):
  """`factory(model, batch_size, nconmax=cap, **kw)` for the first cap of AUTO_NCONMAX whose scratch fits."""
  for cap in AUTO_NCONMAX:
    try:
      return factory(model, batch_size, nconmax=cap, **kw)
    except Exception as e:      # pylint: disable=broad-except
      if cap == AUTO_NCONMAX[-1] or 'does not fit' not in str(e):
        raise


def send_xfrc(state, a):
  """Whether the `xfrc_applied` array `a` goes to the batch whose owner keeps its marks in the dict `state` (a batch that
  was just created: `{}`).  Uploading xfrc_applied switches the kernel's external-force path on for good (6 nbody reals
  per environment per step), and a mere READ of the array makes a facade consider it for upload: all-zero forces are only
  sent once a non-zero one has been, i.e. when there is something to clear."""
  if not np.any(a) and not state.get('_xfrc_sent', False):
    return False
  state['_xfrc_sent'] = True
  return True


def fill_contacts(buf, n, get):
  """The first `n` records of the structured array `buf` from one environment's `contact_*` device fields."""
  for col, width in (('geom1', 1), ('geom2', 1), ('dist', 1), ('pos', 3), ('frame', 9)):
    buf[col][:n] = np.asarray(get('contact_' + col)).reshape(-1, *((width,) if width > 1 else ()))[:n]


# ---------------------------------------------------------------------------------------------------------------------
# row helpers: quaternions (..., 4), vectors (..., 3)
# ---------------------------------------------------------------------------------------------------------------------
def cross(a, b):
  return np.stack([a[..., 1]*b[..., 2] - a[..., 2]*b[..., 1], a[..., 2]*b[..., 0] - a[..., 0]*b[..., 2],
                   a[..., 0]*b[..., 1] - a[..., 1]*b[..., 0]], axis=-1)


def quat_mul_rows(a, b):
  w1, x1, y1, z1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
  w2, x2, y2, z2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
  return np.stack([w1*w2 - x1*x2 - y1*y2 - z1*z2, w1*x2 + x1*w2 + y1*z2 - z1*y2,
                   w1*y2 - x1*z2 + y1*w2 + z1*x2, w1*z2 + x1*y2 - y1*x2 + z1*w2], axis=-1)


def quat_to_mat_rows(q):
  """(..., 4) -> (..., 9), row-major."""
  w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
  return np.stack([w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y),
                   2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x),
                   2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z], axis=-1)


def _mats(q):
  return quat_to_mat_rows(q).reshape(q.shape[:-1] + (3, 3))


def _rot(R, v):
  return np.einsum('...ij,...j->...i', R, v)


# ---------------------------------------------------------------------------------------------------------------------
# per-model plans: index tables that depend on the model's structure only, built once and kept with the compiled model
# ---------------------------------------------------------------------------------------------------------------------
PLAN_ATTR = '_host_plans'


def _plan(c, build):
  plans = c.__dict__.setdefault(PLAN_ATTR, {})
  name = build.__name__
  if name not in plans:
    plans[name] = build(c)
  return plans[name]


def _joint_plan(c):
  """The joints grouped by their rank counted from the LAST joint of their body (pass r of joint_frames handles every
  rank-r joint of the model at once)."""
  rank = np.zeros(c.njnt, dtype=np.int64)
  for b in range(c.nbody):
    j0, jn = int(c.body_jntadr[b]), int(c.body_jntnum[b])
    for k in range(jn):
      rank[j0 + k] = jn - 1 - k
  typ = np.asarray(c.jnt_type, dtype=np.int64)
  passes = []
  for r in range(int(rank.max()) + 1 if c.njnt else 0):
    js = np.nonzero(rank == r)[0]
    passes.append({'j': js, 'b': np.asarray(c.jnt_bodyid, dtype=np.int64)[js], 't': typ[js],
                   'qa': np.asarray(c.jnt_qposadr, dtype=np.int64)[js]})
  return passes


def _dof_plan(c):
  nv = c.nv
  kind = np.zeros(nv, dtype=np.int64)      # 0: world axis (free translation), 1: a column of the body's xmat, 2: the joint's xaxis
  col, jnt, body, rot, fixed_anchor = (np.zeros(nv, dtype=np.int64) for _ in range(5))
  for j in range(c.njnt):
    d, t, b = int(c.jnt_dofadr[j]), int(c.jnt_type[j]), int(c.jnt_bodyid[j])
    n = JNT_NV[t]
    jnt[d:d + n], body[d:d + n] = j, b
    if t == 0:
      kind[d:d + 3], col[d:d + 3] = 0, np.arange(3)
      kind[d + 3:d + 6], col[d + 3:d + 6], rot[d + 3:d + 6], fixed_anchor[d + 3:d + 6] = 1, np.arange(3), 1, 1
    elif t == 1:
      kind[d:d + 3], col[d:d + 3], rot[d:d + 3] = 1, np.arange(3), 1
    else:
      kind[d], rot[d] = 2, int(t == 3)
  return dict(kind=kind, col=col, jnt=jnt, body=body, rot=rot.astype(bool), free_rot=fixed_anchor.astype(bool))


def _body_dofmask(c):
  """mask[b, k]: body b is moved by dof k (k's body is b or an ancestor of b)."""
  anc = np.zeros((c.nbody, c.nv), dtype=bool)
  for b in range(1, c.nbody):
    anc[b] = anc[int(c.body_parentid[b])]
    d0, dn = int(c.body_dofadr[b]), int(c.body_dofnum[b])
    if dn:
      anc[b, d0:d0 + dn] = True
  return anc


def _subtree(c):
  """sub[r, b]: b is in the subtree rooted at r."""
  sub = np.zeros((c.nbody, c.nbody), dtype=bool)
  for b in range(c.nbody):
    a = b
    while True:
      sub[a, b] = True
      if a == 0:
        break
      a = int(c.body_parentid[a])
  return sub


# ---------------------------------------------------------------------------------------------------------------------
# derivations both facades serve
# ---------------------------------------------------------------------------------------------------------------------
def joint_frames(c, qpos, xpos, xquat):
  """mjData.xanchor / xaxis as (anchor, axis), each (..., njnt, 3), from qpos (..., nq) and the device's body frames xpos
  (..., nbody, 3) / xquat (..., nbody, 4).  mj_kinematics takes each joint's anchor and axis in the body frame accumulated
  BEFORE that joint moves it; here the walk runs the other way, from the body's FINAL frame back through its joints: a
  hinge or ball rotation leaves its own anchor and axis where they were, a slide moves the frame along its axis.  One
  vectorised pass per joint rank within a body (at most three in the suite models), over all environments at once.  (A
  mocap body has no joints; its children start from its device frame like any other.)"""
  qpos = np.asarray(qpos, dtype=np.float64)
  lead = qpos.shape[:-1]
  anchor, axis = np.zeros(lead + (c.njnt, 3)), np.zeros(lead + (c.njnt, 3))
  if not c.njnt:
    return anchor, axis
  pos, quat = np.array(xpos, dtype=np.float64), np.array(xquat, dtype=np.float64)      # current frame per body
  jaxis, jpos = np.asarray(c.jnt_axis, dtype=np.float64), np.asarray(c.jnt_pos, dtype=np.float64)
  q0 = np.asarray(c.qpos0, dtype=np.float64)
  for ps in _plan(c, _joint_plan):
    js, bs, ts, qa = ps['j'], ps['b'], ps['t'], ps['qa']
    R = _mats(quat[..., bs, :])
    ax = _rot(R, jaxis[js])
    an = pos[..., bs, :] + _rot(R, jpos[js])
    free, ball, slide, hinge = ts == 0, ts == 1, ts == 2, ts == 3
    if free.any():
      k = np.nonzero(free)[0]
      an[..., k, :] = np.stack([qpos[..., qa[k]], qpos[..., qa[k] + 1], qpos[..., qa[k] + 2]], axis=-1)
      ax[..., k, :] = jaxis[js[k]]
    if slide.any():
      k = np.nonzero(slide)[0]
      shift = ax[..., k, :] * (qpos[..., qa[k]] - q0[qa[k]])[..., None]
      an[..., k, :] -= shift
      pos[..., bs[k], :] -= shift
    rot = hinge | ball
    if rot.any():
      k = np.nonzero(rot)[0]
      qloc = np.zeros(lead + (k.size, 4))
      kh = hinge[k]
      if kh.any():
        ang = (qpos[..., qa[k[kh]]] - q0[qa[k[kh]]]) / 2
        qloc[..., kh, 0] = np.cos(ang)
        qloc[..., kh, 1:] = jaxis[js[k[kh]]] * np.sin(ang)[..., None]
      kb = ~kh
      if kb.any():
        qb = np.stack([qpos[..., qa[k[kb]] + i] for i in range(4)], axis=-1)
        qloc[..., kb, :] = qb / np.linalg.norm(qb, axis=-1, keepdims=True)
      qprev = quat_mul_rows(quat[..., bs[k], :], qloc * np.array([1.0, -1, -1, -1]))
      quat[..., bs[k], :] = qprev
      Rp = _mats(qprev)
      pos[..., bs[k], :] = an[..., k, :] - _rot(Rp, jpos[js[k]])
      if kb.any():      # (a ball joint turns its own nominal axis: mjData.xaxis is the axis BEFORE the joint acts)
        ax[..., k[kb], :] = _rot(Rp[..., kb, :, :], jaxis[js[k[kb]]])
    anchor[..., js, :], axis[..., js, :] = an, ax
  return anchor, axis


def spatial_tendons(c):
  """Ids of the tendons that run through sites (`tendons` needs the site positions and body velocities for these only)."""
  return [t for t in range(c.ntendon) if c.tendon_num[t] and c.wrap_type[c.tendon_adr[t]] != C['DMC_WRAP_JOINT']]


def tendons(c, qpos, qvel, site_xpos=None, cvel=None, subtree_com=None):
  """mjData.ten_length / ten_velocity / wrap_xpos (mj_tendon, mj_fwdVelocity: `ten_velocity = ten_J qvel`) as (length
  (..., ntendon), velocity (..., ntendon), wrap_xpos (..., nwrap, 6)) -- the kernel re-derives the few tendon lengths
  where it needs them and stores none.  Fixed tendons: the coefficient-weighted sum of joint coordinates / velocities;
  site-to-site spatial tendons: the segment lengths, and their rates from the sites' velocities (com-based `cvel` of the
  body, moved to the site).  `site_xpos (..., nsite, 3)`, `cvel (..., nbody, 6)` and `subtree_com (..., nbody, 3)` are read
  only if the model has `spatial_tendons`."""
  qpos, qvel = np.asarray(qpos, dtype=np.float64), np.asarray(qvel, dtype=np.float64)
  lead, nt = qpos.shape[:-1], c.ntendon
  length, velocity, wrap = np.zeros(lead + (nt,)), np.zeros(lead + (nt,)), np.zeros(lead + (c.nwrap, 6))
  spatial = spatial_tendons(c)

  def point(w):
    sid = int(c.wrap_objid[w])
    b = int(c.site_bodyid[sid])
    pos = site_xpos[..., sid, :]
    return pos, cvel[..., b, 3:] + np.cross(cvel[..., b, :3], pos - subtree_com[..., c.body_rootid[b], :])
  for t in range(nt):
    w0, wn = int(c.tendon_adr[t]), int(c.tendon_num[t])
    if t not in spatial:
      for w in range(w0, w0 + wn):
        j = int(c.wrap_objid[w])
        length[..., t] += c.wrap_prm[w] * qpos[..., c.jnt_qposadr[j]]
        velocity[..., t] += c.wrap_prm[w] * qvel[..., c.jnt_dofadr[j]]
      continue
    for w in range(w0, w0 + wn - 1):
      (p0, v0), (p1, v1) = point(w), point(w + 1)
      wrap[..., w, :3], wrap[..., w, 3:] = p0, p1
      dif = p1 - p0
      n = np.linalg.norm(dif, axis=-1)
      length[..., t] += n
      ok = n > MINVAL
      velocity[ok, t] += np.einsum('ek,ek->e', dif[ok] / n[ok, None], (v1 - v0)[ok])
  return length, velocity, wrap


def object_velocity(c, kind, objid, get, local):
  """mj_objectVelocity (wrapper/core.py:500-525): the 6D velocity of a body / xbody / geom / site as (angular, linear),
  each (..., 3), in the world frame or (`local`) the object's own, from the com-based `cvel` of its body.  `kind`: a key of
  OBJECT_KINDS; `get(field, *shape)` reads an mjData array as (..., *shape)."""
  rows, posf, matf = OBJECT_KINDS[kind]
  body = int(objid if rows == 'body' else c.geom_bodyid[objid] if rows == 'geom' else c.site_bodyid[objid])
  n = {'body': c.nbody, 'geom': c.ngeom, 'site': c.nsite}[rows]
  pos = get(posf, n, 3)[..., objid, :]
  if matf is None:
    mat = _mats(quat_mul_rows(get('xquat', c.nbody, 4)[..., objid, :], np.asarray(c.body_iquat[objid], dtype=np.float64)))
  else:
    mat = get(matf, n, 3, 3)[..., objid, :, :]
  cvel = get('cvel', c.nbody, 6)[..., body, :]
  com = get('subtree_com', c.nbody, 3)[..., int(c.body_rootid[body]), :]
  ang = cvel[..., :3]
  lin = cvel[..., 3:] - np.cross(pos - com, ang)
  if local:
    ang, lin = np.einsum('...ij,...i->...j', mat, ang), np.einsum('...ij,...i->...j', mat, lin)
  return ang, lin


CONTACT_ABOUT = ('com', 'origin', 'world')


def _contact_ids(c, key, kind, count):
  keys = key if isinstance(key, (list, tuple)) else [key]
  if not keys:
    raise ValueError('target: an empty list of %ss' % kind)
  out = []
  for k in keys:
    if isinstance(k, str):
      out.append(int(c.name2id(k, kind)))      # (ValueError: no such name)
    elif isinstance(k, (int, np.integer)) and not isinstance(k, bool):
      if not 0 <= int(k) < count:
        raise ValueError('target: %s id %d out of range (the model has %d)' % (kind, int(k), count))
      out.append(int(k))
    else:
      raise ValueError('target: a %s is named by a string or an id, got %r' % (kind, k))
  return out


def contact_geom_set(c, spec):
  """(mask (ngeom,) bool, named body) of a set of geoms: a geom name or id, dict(geom=..), dict(body=..) -- the body's own
  geoms -- or dict(body=.., subtree=True) -- those of the body and everything below it.  A name, an id or a list of them.
  The named body is the (first) body, or the (first) geom's body."""
  if isinstance(spec, (str, int, np.integer)) and not isinstance(spec, bool):
    spec = dict(geom=spec)
  if not isinstance(spec, dict) or not ({'geom'} == set(spec) or ('body' in spec and set(spec) <= {'body', 'subtree'})):
    raise ValueError('target: expected a geom name or id, dict(geom=..) or dict(body=..[, subtree=True]), got %r' % (spec,))
  mask = np.zeros(c.ngeom, dtype=bool)
  gbody = np.asarray(c.geom_bodyid, dtype=np.int64).reshape(-1)
  if 'geom' in spec:
    ids = _contact_ids(c, spec['geom'], 'geom', c.ngeom)
    mask[ids] = True
    return mask, int(gbody[ids[0]])
  bodies = _contact_ids(c, spec['body'], 'body', c.nbody)
  inb = np.zeros(c.nbody, dtype=bool)
  inb[bodies] = True
  if spec.get('subtree'):
    inb = _plan(c, _subtree)[bodies].any(axis=0)
  mask[:] = inb[gbody]
  return mask, bodies[0]


def contact_targets(c, targets):
  """[dict(S, O (ngeom,) bool, body)] of a list of contact targets: a geom set (contact_geom_set) and, in a dict,
  `other=` a second one that filters the partner geom (default: every geom).  A set without a geom is refused."""
  targets = list(targets) if isinstance(targets, (list, tuple)) else [targets]
  if not targets:
    raise ValueError('targets: at least one target is needed')
  out = []
  for t in targets:
    other = None
    if isinstance(t, dict) and 'other' in t:
      t = dict(t)
      other = t.pop('other')
    S, body = contact_geom_set(c, t)
    O = np.ones(c.ngeom, dtype=bool) if other is None else contact_geom_set(c, other)[0]
    if not S.any():
      raise ValueError('target %r: the set of geoms is empty' % (t,))
    out.append(dict(S=S, O=O, body=body))
  return out


def contact_wrenches(c, get, targets, about='com', local=False):
  """The net contact wrench on every target from the `contact_*` arrays of the last forward: dict(force, torque
  (..., T, 3), normal, dist (..., T), count (..., T) int32).  Contact k between geom1 and geom2 pushes geom2's body with
  f = frame' contact_force[0:3] (torque about the contact point: frame' contact_force[3:6]) and geom1's body with the
  opposite; a contact counts for a target with +1 when geom2 is in its set S, geom1 in its filter O and not in S, with -1 the
  other way round.  torque is taken about the named body's xipos ('com'), xpos ('origin') or 0 ('world'); `local` rotates
  force and torque into the named body's frame.  `get(field, *shape)` reads an mjData array as (..., *shape)."""
  if about not in CONTACT_ABOUT:
    raise ValueError('about must be one of %s, got %r' % (CONTACT_ABOUT, about))
  tg = contact_targets(c, targets)
  ncon = np.asarray(get('ncon', 1)).astype(np.int64)[..., 0]
  g1, g2 = (np.asarray(get('contact_geom' + k, -1)).astype(np.int64) for k in '12')
  K = g1.shape[-1]
  frame, lf = np.asarray(get('contact_frame', K, 3, 3), dtype=np.float64), np.asarray(get('contact_force', K, 6), dtype=np.float64)
  pos, dist = np.asarray(get('contact_pos', K, 3), dtype=np.float64), np.asarray(get('contact_dist', K), dtype=np.float64)
  live = (np.arange(K) < ncon[..., None]) & (g1 >= 0) & (g2 >= 0) & (g1 < c.ngeom) & (g2 < c.ngeom)
  a, b = np.where(live, g1, 0), np.where(live, g2, 0)
  f = np.einsum('...kij,...ki->...kj', frame, lf[..., :3])
  t = np.einsum('...kij,...ki->...kj', frame, lf[..., 3:])
  out = dict(force=[], torque=[], normal=[], count=[], dist=[])
  for d in tg:
    S, O, body = d['S'], d['O'], d['body']
    plus, minus = live & S[b] & O[a] & ~S[a], live & S[a] & O[b] & ~S[b]
    s = plus.astype(np.float64) - minus
    hit = plus | minus
    r = 0.0 if about == 'world' else np.asarray(get('xipos' if about == 'com' else 'xpos', c.nbody, 3), dtype=np.float64)[..., body, :][..., None, :]
    force = (s[..., None]*f).sum(axis=-2)
    torque = (s[..., None]*(t + cross(pos - r, f))).sum(axis=-2)
    if local:
      R = np.asarray(get('xmat', c.nbody, 3, 3), dtype=np.float64)[..., body, :, :]
      force, torque = np.einsum('...ij,...i->...j', R, force), np.einsum('...ij,...i->...j', R, torque)
    out['force'].append(force)
    out['torque'].append(torque)
    out['normal'].append((hit*lf[..., 0]).sum(axis=-1))
    out['count'].append(hit.sum(axis=-1).astype(np.int32))
    out['dist'].append(np.where(hit, dist, np.inf).min(axis=-1) if K else np.full(ncon.shape, np.inf))
  return {k: np.stack(v, axis=-2 if k in ('force', 'torque') else -1) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# derivations only MjData serves (one environment)
# ---------------------------------------------------------------------------------------------------------------------
def dof_axes(c, xpos, xmat, xanchor, xaxis):
  """Per dof: its world axis (nv, 3), the point its rotation passes through (nv, 3) and whether it rotates (nv,) -- a
  hinge's or slide's joint axis, the columns of the body's orientation for a ball joint and the rotations of a free
  joint, the world axes for a free joint's translations (mj_comPos's cdof, in world terms)."""
  p = _plan(c, _dof_plan)
  R = np.asarray(xmat, dtype=np.float64).reshape(c.nbody, 3, 3)
  axis = np.where((p['kind'] == 2)[:, None], xaxis[p['jnt']], R[p['body'], :, p['col']])
  axis = np.where((p['kind'] == 0)[:, None], np.eye(3)[p['col']], axis)
  anchor = np.where(p['free_rot'][:, None], xpos[p['body']], xanchor[p['jnt']])
  return axis, anchor, p['rot']


def point_jacobian(c, body, point, xpos, xmat, xanchor, xaxis):
  """mj_jac: (jacp (3, nv), jacr (3, nv)) of the world point `point` moving with body `body`."""
  axis, anchor, rot = dof_axes(c, xpos, xmat, xanchor, xaxis)
  mask = _plan(c, _body_dofmask)[int(body)]
  r = np.asarray(point, dtype=np.float64)[None, :] - anchor
  jp = np.where(rot[:, None], cross(axis, r), axis) * mask[:, None]
  jr = np.where(rot[:, None], axis, 0.0) * mask[:, None]
  return jp.T.copy(), jr.T.copy()


def _quat_integrate(q, v, dt):
  """mju_quatIntegrate: q (4,) turned by the local angular velocity v (3,) over dt."""
  n = np.linalg.norm(v)
  ax = v / n if n >= MINVAL else np.array([1.0, 0, 0])
  ang = dt * n
  qn = np.linalg.norm(q)
  q = np.array([1.0, 0, 0, 0]) if qn < MINVAL else q / qn if abs(qn - 1) > MINVAL else q
  return quat_mul_rows(q, np.concatenate([[np.cos(ang / 2)], ax * np.sin(ang / 2)]))


def integrate_pos(c, qpos, qvel, dt):
  """mj_integratePos: `qpos` (nq,) advanced in place by `qvel` (nv,) over dt; ball and free rotations compose on the
  right, in local axes."""
  for j in range(c.njnt):
    t, a, d = int(c.jnt_type[j]), int(c.jnt_qposadr[j]), int(c.jnt_dofadr[j])
    if t == 0:
      qpos[a:a + 3] += dt * qvel[d:d + 3]
      qpos[a + 3:a + 7] = _quat_integrate(qpos[a + 3:a + 7], qvel[d + 3:d + 6], dt)
    elif t == 1:
      qpos[a:a + 4] = _quat_integrate(qpos[a:a + 4], qvel[d:d + 3], dt)
    else:
      qpos[a] += dt * qvel[d]


def _quat_sub(qa, qb):
  """mju_subQuat: the local rotation vector that takes qb to qa."""
  q = quat_mul_rows(qb * np.array([1.0, -1, -1, -1]), qa)
  ax = q[1:4].copy()
  s = np.linalg.norm(ax)
  ax = ax / s if s >= MINVAL else np.array([1.0, 0, 0])
  ang = 2 * np.arctan2(s, q[0])
  if ang > np.pi:
    ang -= 2 * np.pi
  return ax * ang


def differentiate_pos(c, qvel, dt, qpos1, qpos2):
  """mj_differentiatePos: `qvel` (nv,) := (qpos2 - qpos1) / dt, the inverse of integrate_pos."""
  for j in range(c.njnt):
    t, a, d = int(c.jnt_type[j]), int(c.jnt_qposadr[j]), int(c.jnt_dofadr[j])
    if t == 0:
      qvel[d:d + 3] = (qpos2[a:a + 3] - qpos1[a:a + 3]) / dt
      qvel[d + 3:d + 6] = _quat_sub(qpos2[a + 3:a + 7], qpos1[a + 3:a + 7]) / dt
    elif t == 1:
      qvel[d:d + 3] = _quat_sub(qpos2[a:a + 4], qpos1[a:a + 4]) / dt
    else:
      qvel[d] = (qpos2[a] - qpos1[a]) / dt


def transition_fd(c, state, step, eps, centered, ctrlrange=None):
  """mjd_transitionFD for one environment: (A, B, C, D) of x' ~ A dx + B du, y ~ C dx + D du by finite differences, with
  x = [dq (nv), qvel (nv), act (na)].  `state`: dict(qpos, qvel, act, ctrl) at the nominal point; `step(qpos, qvel, act,
  ctrl)` returns (qpos', qvel', act', sensordata) of one transition from that state, everything else held at the nominal
  values by the caller.  Positions are nudged with integrate_pos and differenced with differentiate_pos; a control is
  nudged only where ctrl and ctrl +- eps lie inside `ctrlrange` (default: the model's) of a ctrllimited actuator -- central
  with both nudges, one-sided against the nominal next state with one, a zero column with none; not centred: the forward
  nudge, or the backward one where the forward one is out.  The batch form is linearize.BatchLinearization."""
  nv, na, nu = int(c.nv), int(c.na), int(c.nu)
  nx = 2 * nv + na
  base = [np.array(state[k], dtype=np.float64).ravel() for k in ('qpos', 'qvel', 'act', 'ctrl')]
  cr = np.asarray(c.actuator_ctrlrange if ctrlrange is None else ctrlrange, dtype=np.float64).reshape(-1, 2)

  def nudged(j, h):
    q, v, a, u = (x.copy() for x in base)
    if j < nv:
      dq = np.zeros(nv)
      dq[j] = 1.0
      integrate_pos(c, q, dq, h)
    elif j < 2 * nv:
      v[j - nv] += h
    elif j < nx:
      a[j - 2 * nv] += h
    else:
      u[j - nx] += h
    return step(q, v, a, u)

  def quotient(hi, lo, h):
    dq = np.zeros(nv)
    differentiate_pos(c, dq, h, lo[0], hi[0])
    return np.concatenate([dq, (hi[1] - lo[1]) / h, (hi[2] - lo[2]) / h]), (hi[3] - lo[3]) / h

  nominal = None
  cols, sens = [], []
  for j in range(nx + nu):
    fwd, back = True, bool(centered)
    if j >= nx and int(c.actuator_ctrllimited[j - nx]):
      u, (lo, hi) = base[3][j - nx], cr[j - nx]
      inside = lambda x: lo <= x <= hi      # pylint: disable=cell-var-from-loop
      fwd = inside(u) and inside(u + eps)
      back = (bool(centered) or not fwd) and inside(u) and inside(u - eps)
    if (fwd != back or not (fwd or back)) and nominal is None:
      nominal = step(*(x.copy() for x in base))
    if fwd and back:
      col = quotient(nudged(j, eps), nudged(j, -eps), 2 * eps)
    elif fwd:
      col = quotient(nudged(j, eps), nominal, eps)
    elif back:
      col = quotient(nominal, nudged(j, -eps), eps)
    else:
      col = (np.zeros(nx), np.zeros_like(nominal[3]))
    cols.append(col[0])
    sens.append(col[1])
  AB = np.stack(cols, axis=1)
  CD = np.stack(sens, axis=1)
  return AB[:, :nx], AB[:, nx:], CD[:, :nx], CD[:, nx:]


def mass_matrix(c, xpos, xmat, xipos, ximat, xanchor, xaxis):
  """Dense joint-space inertia M(q) (what mj_crb leaves in mjData.M) from world-frame body Jacobians:
  M = sum_b m_b Jp_b' Jp_b + Jr_b' (R_b I_b R_b') Jr_b + diag(dof_armature)."""
  nv, nb = c.nv, c.nbody
  axis, anchor, rot = dof_axes(c, xpos, xmat, xanchor, xaxis)
  mask = _plan(c, _body_dofmask)                             # (nb, nv)
  r = xipos[:, None, :] - anchor[None, :, :]                 # (nb, nv, 3)
  jp = np.where(rot[None, :, None], cross(np.broadcast_to(axis[None, :, :], r.shape), r), axis[None, :, :]) * mask[:, :, None]
  jr = np.where(rot[None, :, None], axis[None, :, :], 0.0) * mask[:, :, None]
  Ri = np.asarray(ximat, dtype=np.float64).reshape(nb, 3, 3)
  jl = np.einsum('bji,bkj->bki', Ri, jr)                     # angular Jacobian in the inertial frame: (nb, nv, 3)
  M = np.einsum('b,bki,bli->kl', np.asarray(c.body_mass, dtype=np.float64), jp, jp)
  M += np.einsum('bki,bi,bli->kl', jl, np.asarray(c.body_inertia, dtype=np.float64), jl)
  M[np.diag_indices(nv)] += np.asarray(c.dof_armature, dtype=np.float64)
  return M


def rne(c, qpos, qvel, qacc, xpos, xquat, xipos, ximat):
  """mj_rne (after mj_comVel) in numpy for one environment: the bias forces c(q, qvel) -- Coriolis, centrifugal, gravity
  unless disabled -- or, with `qacc`, M qacc + c: inverse dynamics of the rigid-body terms, `dof_armature * qacc`
  included (mj_rne itself leaves the armature to its callers).  No passive, actuator or constraint force.  Poses arrive
  as for `mass_matrix` (xpos (nbody, 3), xquat (nbody, 4), xipos, ximat (nbody, 9)); the joint frames are derived from
  `qpos`.  Spatial vectors are (angular, linear) about the world origin."""
  nv, nb = c.nv, c.nbody
  qvel = np.asarray(qvel, dtype=np.float64).ravel()
  acc = np.zeros(nv) if qacc is None else np.asarray(qacc, dtype=np.float64).ravel()
  xpos, xquat = np.asarray(xpos, dtype=np.float64).reshape(nb, 3), np.asarray(xquat, dtype=np.float64).reshape(nb, 4)
  xipos, Ri = np.asarray(xipos, dtype=np.float64).reshape(nb, 3), np.asarray(ximat, dtype=np.float64).reshape(nb, 3, 3)
  anchor, jaxis = joint_frames(c, np.asarray(qpos, dtype=np.float64), xpos, xquat)
  axis, point, rot = dof_axes(c, xpos, quat_to_mat_rows(xquat), anchor, jaxis)
  cdof = np.where(rot[:, None], np.concatenate([axis, cross(axis, -point)], axis=1), np.concatenate([np.zeros((nv, 3)), axis], axis=1))
  xm = lambda v, w: np.concatenate([np.cross(v[:3], w[:3]), np.cross(v[:3], w[3:]) + np.cross(v[3:], w[:3])])      # v x w (motion)
  xf = lambda v, f: np.concatenate([np.cross(v[:3], f[:3]) + np.cross(v[3:], f[3:]), np.cross(v[:3], f[3:])])      # v x* f (force)

  def inertia(b, v):      # the body's spatial inertia about the origin times a motion vector
    m, com = float(c.body_mass[b]), xipos[b]
    vc = v[3:] + np.cross(v[:3], com)      # the velocity of the centre of mass
    return np.concatenate([Ri[b] @ (np.asarray(c.body_inertia[b], dtype=np.float64) * (Ri[b].T @ v[:3])) + m * np.cross(com, vc), m * vc])
  g = np.zeros(3) if int(c.opt.disableflags) & C['DMC_DSBL_GRAVITY'] else np.asarray(c.opt.gravity, dtype=np.float64)
  cvel, cacc, cfrc = np.zeros((nb, 6)), np.zeros((nb, 6)), np.zeros((nb, 6))
  cacc[0, 3:] = -g
  for b in range(1, nb):
    p = int(c.body_parentid[b])
    v, a = cvel[p].copy(), cacc[p].copy()
    for j in range(int(c.body_jntadr[b]), int(c.body_jntadr[b]) + int(c.body_jntnum[b])):
      t, d = int(c.jnt_type[j]), int(c.jnt_dofadr[j])
      if t == 0:      # the translations of a free joint: constant axes
        for k in range(d, d + 3):
          v += cdof[k] * qvel[k]
          a += cdof[k] * acc[k]
        d += 3
      n = 3 if t in (0, 1) else 1
      carried = v.copy()      # what carries the joint's axes: everything before the joint (mj_comVel)
      for k in range(d, d + n):
        v += cdof[k] * qvel[k]
        a += xm(carried, cdof[k]) * qvel[k] + cdof[k] * acc[k]
    cvel[b], cacc[b] = v, a
    cfrc[b] = inertia(b, a) + xf(v, inertia(b, v))
  for b in range(nb - 1, 0, -1):
    cfrc[int(c.body_parentid[b])] += cfrc[b]
  body = _plan(c, _dof_plan)['body']
  return np.einsum('ki,ki->k', cdof, cfrc[body]) + np.asarray(c.dof_armature, dtype=np.float64) * acc


def passive(c, qpos, qvel):
  """mjData.qfrc_passive (mj_passive): joint springs and dampers, fixed-tendon springs and dampers.  Fluid forces and
  ball / free joint springs are computed on the device only: a model that has them is refused here rather than served a
  partial sum."""
  if float(c.opt.density) or float(c.opt.viscosity):
    raise NotImplementedError('mjData.qfrc_passive of a model with fluid forces is not derived on the host')
  flags = int(c.opt.disableflags)
  out = np.zeros(c.nv)
  if not flags & C['DMC_DSBL_DAMPER']:
    out -= np.asarray(c.dof_damping, dtype=np.float64) * qvel
  if not flags & C['DMC_DSBL_SPRING']:
    for j in range(c.njnt):
      k = float(c.jnt_stiffness[j])
      if not k:
        continue
      if c.jnt_type[j] not in (2, 3):
        raise NotImplementedError('mjData.qfrc_passive with a spring on a ball / free joint is not derived on the host')
      out[c.jnt_dofadr[j]] -= k * (qpos[c.jnt_qposadr[j]] - c.qpos_spring[c.jnt_qposadr[j]])
  for t in range(c.ntendon):
    ks, kd = float(c.tendon_stiffness[t]), float(c.tendon_damping[t])
    if not (ks or kd):
      continue
    w0, wn = int(c.tendon_adr[t]), int(c.tendon_num[t])
    js = [int(c.wrap_objid[w]) for w in range(w0, w0 + wn)]
    coef = np.asarray(c.wrap_prm[w0:w0 + wn], dtype=np.float64)
    length = float(coef @ qpos[np.asarray(c.jnt_qposadr)[js]])
    vel = float(coef @ qvel[np.asarray(c.jnt_dofadr)[js]])
    f = 0.0
    if ks and not flags & C['DMC_DSBL_SPRING']:
      f -= ks * (length - float(c.tendon_lengthspring[t]))
    if kd and not flags & C['DMC_DSBL_DAMPER']:
      f -= kd * vel
    out[np.asarray(c.jnt_dofadr)[js]] += coef * f
  return out


def act_dot(c, actadr, ctrl, act):
  """mjData.act_dot (mj_fwdActuation): integrator `ctrl`, filter `(ctrl - act) / tau`; filterexact has the same rate.
  `actadr`: mjModel.actuator_actadr."""
  out = np.zeros(c.na)
  for i in range(c.nu):
    if actadr[i] < 0:
      continue
    u = ctrl[i]
    if c.actuator_ctrllimited[i] and not int(c.opt.disableflags) & C['DMC_DSBL_CLAMPCTRL']:
      u = min(max(u, c.actuator_ctrlrange[i, 0]), c.actuator_ctrlrange[i, 1])
    if int(c.actuator_dyntype[i]) == C['DMC_DYN_INTEGRATOR']:
      out[actadr[i]] = u
    else:
      out[actadr[i]] = (u - act[actadr[i]]) / max(MINVAL, c.actuator_dynprm[i, 0])
  if int(c.opt.disableflags) & C['DMC_DSBL_ACTUATION']:
    out[:] = 0
  return out


def subtree_vel(c, cvel, subtree_com, xipos, ximat=None):
  """mj_subtreeVel as (subtree_linvel, subtree_angmom | None without `ximat`): linear velocity of every subtree's centre
  of mass and its angular momentum about it, from the device's com-based body velocities."""
  nb = c.nbody
  mass = np.asarray(c.body_mass, dtype=np.float64)
  sub = _plan(c, _subtree).astype(np.float64)                     # (root, body)
  ang = cvel[:, :3]
  lin = cvel[:, 3:] + cross(ang, xipos - subtree_com[np.asarray(c.body_rootid)])      # velocity of each body's own COM
  msub = np.maximum(sub @ mass, MINVAL)
  vsub = (sub @ (mass[:, None] * lin)) / msub[:, None]
  if ximat is None:
    return vsub, None
  R = ximat.reshape(nb, 3, 3)
  spin = np.einsum('bij,bj,bkj,bk->bi', R, np.asarray(c.body_inertia, dtype=np.float64), R, ang)
  # sum_b [I w + m (x - X) x (v - V)] = sum_b [I w + m x x v] - M X x V   (X, V: the subtree's centre of mass and its velocity)
  own = spin + mass[:, None] * cross(xipos, lin)
  return vsub, sub @ own - msub[:, None] * cross(subtree_com, vsub)


# ---------------------------------------------------------------------------------------------------------------------
# mj_ray on the host: one environment, numpy.  The device form is csrc/ray_core.h (rays.BatchRays); the rules are stated
# once, in PARITY_ASSUMPTIONS.md rows 58-60.
# ---------------------------------------------------------------------------------------------------------------------
_RAY_TYPES = tuple(C['DMC_GEOM_' + n] for n in ('PLANE', 'SPHERE', 'CAPSULE', 'ELLIPSOID', 'CYLINDER', 'BOX'))


def _ray_roots(q, v, r2):
  """Roots x0 <= x1 of |q + x v|^2 = r2 through the point of closest approach, or None."""
  a = float(v @ v)
  if a < MINVAL:
    return None
  t0 = -float(q @ v) / a
  p = q + t0 * v
  cc = float(p @ p) - r2
  if cc > 0:
    return None
  h = np.sqrt(-cc / a)
  return t0 - h, t0 + h


def _ray_primitive(gtype, s, lp, lv):
  """Nearest x >= 0 of lp + x lv on one primitive in its own frame, or -1."""
  PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = _RAY_TYPES
  cands = []
  if gtype == PLANE:
    if lv[2] > -MINVAL:
      return -1.0
    x = -lp[2] / lv[2]
    p = lp + x * lv
    ok = x >= 0 and (s[0] <= 0 or abs(p[0]) <= s[0]) and (s[1] <= 0 or abs(p[1]) <= s[1])
    return float(x) if ok else -1.0
  if gtype == SPHERE:
    cands = list(_ray_roots(lp, lv, s[0] * s[0]) or ())
  elif gtype == ELLIPSOID:
    cands = list(_ray_roots(lp / s, lv / s, 1.0) or ())
  elif gtype in (CAPSULE, CYLINDER):
    for x in _ray_roots(lp[:2], lv[:2], s[0] * s[0]) or ():
      if abs(lp[2] + x * lv[2]) <= s[1]:
        cands.append(x)
    for sg in (1.0, -1.0):
      if gtype == CAPSULE:
        for x in _ray_roots(lp - [0, 0, sg * s[1]], lv, s[0] * s[0]) or ():
          if sg * (lp[2] + x * lv[2]) >= s[1]:
            cands.append(x)
      elif abs(lv[2]) >= MINVAL:
        x = (sg * s[1] - lp[2]) / lv[2]
        p = lp + x * lv
        if p[0] * p[0] + p[1] * p[1] <= s[0] * s[0]:
          cands.append(x)
  elif gtype == BOX:
    for ax in range(3):
      if abs(lv[ax]) < MINVAL:
        continue
      for sg in (-1.0, 1.0):
        x = (sg * s[ax] - lp[ax]) / lv[ax]
        p = lp + x * lv
        if all(abs(p[k]) <= s[k] for k in range(3) if k != ax):
          cands.append(x)
  cands = [float(x) for x in cands if x >= 0]
  return min(cands) if cands else -1.0


def ray_filter(c, geomgroup=None, flg_static=1):
  """(ngeom) bool: the geoms a ray can hit at all -- primitives (meshes and height fields are scenery), visible (the
  compiler's geom_invisible: alpha 0 on the geom or its material), their group's flag set (groups clamped to 0..5;
  geomgroup None: every group), and, with flg_static 0, not on a body welded to the world."""
  ok = np.isin(np.asarray(c.geom_type), _RAY_TYPES) & ~np.asarray(c.geom_invisible, dtype=bool)
  if geomgroup is not None:
    flags = np.asarray(geomgroup).reshape(-1)
    if flags.size != 6:
      raise ValueError('geomgroup must hold six flags (or be None)')
    ok &= flags[np.clip(np.asarray(c.geom_group, dtype=np.int64), 0, 5)] != 0
  if not flg_static:
    ok &= np.asarray(c.body_weldid)[np.asarray(c.geom_bodyid)] != 0
  return ok


def ray_cast(c, geom_xpos, geom_xmat, geom_size, pnt, vec, geomgroup=None, flg_static=1, bodyexclude=-1):
  """mj_ray for one environment: (x, geom id) of the nearest hit of pnt + x vec, x >= 0 in units of |vec|; (-1, -1) when
  nothing is hit.  geom_xpos (ngeom, 3), geom_xmat (ngeom, 9), geom_size (ngeom, 3): the poses and sizes in force."""
  gpos = np.asarray(geom_xpos, dtype=np.float64).reshape(-1, 3)
  gmat = np.asarray(geom_xmat, dtype=np.float64).reshape(-1, 3, 3)
  size = np.asarray(geom_size, dtype=np.float64).reshape(-1, 3)
  pnt = np.asarray(pnt, dtype=np.float64).reshape(3)
  vec = np.asarray(vec, dtype=np.float64).reshape(3)
  ok = ray_filter(c, geomgroup, flg_static)
  best, gid = -1.0, -1
  for g in np.nonzero(ok)[0]:
    if int(c.geom_bodyid[g]) == int(bodyexclude):
      continue
    x = _ray_primitive(int(c.geom_type[g]), size[g], gmat[g].T @ (pnt - gpos[g]), gmat[g].T @ vec)
    if x >= 0 and (gid < 0 or x < best):
      best, gid = x, int(g)
  return best, gid

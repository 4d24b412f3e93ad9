/* dmc_model_layout.h -- the flat "compiled model" blob that crosses the C-ABI.
 *
 * The reference hands MuJoCo an MJCF string and gets back an opaque mjModel
 * (dm_control/mujoco/wrapper/core.py:151-182, MjModel.from_xml_string).  MuJoCo's
 * XML compiler is third-party and absent, so this repo's own MJCF compiler
 * (dm_control_amd/mjcf_compiler.py) produces the constant tables below, named
 * after the mjModel fields the reference reads (dm_control/mujoco/index.py:93-174).
 *
 * Blob format (two flat arrays):
 *   ints  = [DMC_MODEL_MAGIC, DMC_MODEL_VERSION, <header ints>, <int fields...>]
 *   reals = [<header reals>, <real fields...>]           (always float64)
 * Field order is exactly the order of the X-macro lists in this file; the
 * Python packer parses this header, so this file is the single source of truth.
 *
 * Count expressions use the header size names (nq, nv, ...).
 */
#ifndef DMC_MODEL_LAYOUT_H_
#define DMC_MODEL_LAYOUT_H_

#define DMC_MODEL_MAGIC   0x444D4331  /* 'DMC1' */
#define DMC_MODEL_VERSION 12

/* ---- header ints (sizes, then options) --------------------------------- */
#define DMC_MODEL_HEADER_INTS(X) \
  X(nq) X(nv) X(nu) X(na) X(nbody) X(njnt) X(ngeom) X(nsite) \
  X(nsensor) X(nsensordata) X(npair) X(nkey) X(ntendon) X(nwrap) X(neq) X(nmocap) \
  X(opt_integrator) X(opt_cone) X(opt_solver) X(opt_iterations) \
  X(opt_ls_iterations) X(opt_noslip_iterations) \
  X(opt_disableflags) X(opt_enableflags)

/* ---- header reals ------------------------------------------------------- */
#define DMC_MODEL_HEADER_REALS(X) \
  X(opt_timestep) X(opt_gravity_x) X(opt_gravity_y) X(opt_gravity_z) \
  X(opt_impratio) X(opt_tolerance) X(opt_ls_tolerance) X(opt_noslip_tolerance) \
  X(opt_density) X(opt_viscosity) X(stat_meaninertia)

/* ---- int fields: X(name, count_expr) ------------------------------------ */
#define DMC_MODEL_INT_FIELDS(X) \
  X(body_parentid, nbody) X(body_rootid, nbody) X(body_weldid, nbody) \
  X(body_jntadr, nbody) X(body_jntnum, nbody) X(body_dofadr, nbody) \
  X(body_dofnum, nbody) X(body_geomadr, nbody) X(body_geomnum, nbody) \
  X(body_mocapid, nbody)   /* row of mjData.mocap_pos / mocap_quat that poses the body, -1: not a mocap body (mujoco/index.py:177-267) */ \
  X(jnt_type, njnt) X(jnt_qposadr, njnt) X(jnt_dofadr, njnt) \
  X(jnt_bodyid, njnt) X(jnt_limited, njnt) \
  X(dof_bodyid, nv) X(dof_jntid, nv) X(dof_parentid, nv) \
  X(geom_type, ngeom) X(geom_contype, ngeom) X(geom_conaffinity, ngeom) \
  X(geom_condim, ngeom) X(geom_bodyid, ngeom) X(geom_priority, ngeom) X(geom_invisible, ngeom) \
  X(site_bodyid, nsite) X(site_type, nsite) \
  X(actuator_trntype, nu) X(actuator_dyntype, nu) X(actuator_gaintype, nu) \
  X(actuator_biastype, nu) X(actuator_trnid, 2*nu) \
  X(actuator_ctrllimited, nu) X(actuator_forcelimited, nu) \
  X(actuator_actlimited, nu)   /* activation clamped to actuator_actrange when it is advanced (mj_nextActivation) */ \
  X(sensor_type, nsensor) X(sensor_objtype, nsensor) X(sensor_objid, nsensor) \
  X(sensor_adr, nsensor) X(sensor_dim, nsensor) X(sensor_needstage, nsensor) \
  X(sensor_reftype, nsensor) X(sensor_refid, nsensor)   /* reference frame of frame{pos,quat,?axis} sensors (mjtObj, id); refid = -1: world */ \
  X(pair_geom1, npair) X(pair_geom2, npair) \
  X(tendon_adr, ntendon) X(tendon_num, ntendon) /* fixed tendons: wraps [adr, adr + num) */ \
  X(wrap_objid, nwrap)                           /* joint id (fixed) or site id (spatial) of each wrap */ \
  X(wrap_type, nwrap) X(tendon_limited, ntendon) \
  X(eq_type, neq) X(eq_obj1id, neq) X(eq_obj2id, neq) X(eq_active0, neq)   /* equality constraints: bodies (connect, weld), joints, a fixed tendon; obj2 = -1: none / world = 0 */

/* ---- real fields: X(name, count_expr) ----------------------------------- */
#define DMC_MODEL_REAL_FIELDS(X) \
  X(qpos0, nq) X(qpos_spring, nq) \
  X(body_pos, 3*nbody) X(body_quat, 4*nbody) X(body_ipos, 3*nbody) \
  X(body_iquat, 4*nbody) X(body_mass, nbody) X(body_subtreemass, nbody) \
  X(body_inertia, 3*nbody) X(body_invweight0, 2*nbody) \
  X(jnt_pos, 3*njnt) X(jnt_axis, 3*njnt) X(jnt_stiffness, njnt) \
  X(jnt_range, 2*njnt) X(jnt_margin, njnt) X(jnt_solref, 2*njnt) \
  X(jnt_solimp, 5*njnt) \
  X(dof_armature, nv) X(dof_damping, nv) X(dof_invweight0, nv) \
  X(dof_frictionloss, nv) X(dof_solref, 2*nv) X(dof_solimp, 5*nv) \
  X(geom_size, 3*ngeom) X(geom_pos, 3*ngeom) X(geom_quat, 4*ngeom) \
  X(geom_friction, 3*ngeom) X(geom_solmix, ngeom) X(geom_solref, 2*ngeom) \
  X(geom_solimp, 5*ngeom) X(geom_margin, ngeom) X(geom_gap, ngeom) \
  X(geom_rbound, ngeom) \
  X(site_size, 3*nsite) X(site_pos, 3*nsite) X(site_quat, 4*nsite) \
  X(actuator_gear, 6*nu) X(actuator_ctrlrange, 2*nu) \
  X(actuator_forcerange, 2*nu) X(actuator_actrange, 2*nu) X(actuator_gainprm, 10*nu) \
  X(actuator_biasprm, 10*nu) X(actuator_dynprm, 10*nu) \
  X(sensor_cutoff, nsensor) X(wrap_prm, nwrap) \
  X(tendon_stiffness, ntendon) X(tendon_damping, ntendon) X(tendon_lengthspring, ntendon) \
  X(tendon_range, 2*ntendon) X(tendon_margin, ntendon) X(tendon_solref_lim, 2*ntendon) \
  X(tendon_solimp_lim, 5*ntendon) X(tendon_invweight0, ntendon) X(tendon_length0, ntendon) \
  X(eq_solref, 2*neq) X(eq_solimp, 5*neq) X(eq_data, 11*neq) /* mjModel.eq_data rows: connect anchor1(3) anchor2(3); weld anchor2(3) anchor1(3) relquat(4) torquescale; joint / tendon polycoef(5) */ \
  X(key_qpos, nq*nkey) X(key_qvel, nv*nkey) X(key_ctrl, nu*nkey) \
  X(key_time, nkey) X(key_act, na*nkey) X(key_mpos, 3*nmocap*nkey) X(key_mquat, 4*nmocap*nkey)   /* the rest of mj_resetDataKeyframe (engine.py:323) */

/* ---- enums (values follow MuJoCo's mjt* enums as the reference re-exports
 * them, dm_control/mujoco/__init__.py:26; only the subset in use) ---------- */
enum { DMC_JNT_FREE = 0, DMC_JNT_BALL = 1, DMC_JNT_SLIDE = 2, DMC_JNT_HINGE = 3 };
enum { DMC_GEOM_PLANE = 0, DMC_GEOM_HFIELD = 1, DMC_GEOM_SPHERE = 2,
       DMC_GEOM_CAPSULE = 3, DMC_GEOM_ELLIPSOID = 4, DMC_GEOM_CYLINDER = 5,
       DMC_GEOM_BOX = 6, DMC_GEOM_MESH = 7 };
enum { DMC_INT_EULER = 0, DMC_INT_RK4 = 1, DMC_INT_IMPLICIT = 2,
       DMC_INT_IMPLICITFAST = 3 };
enum { DMC_CONE_PYRAMIDAL = 0, DMC_CONE_ELLIPTIC = 1 };
enum { DMC_SOL_PGS = 0, DMC_SOL_CG = 1, DMC_SOL_NEWTON = 2 };
enum { DMC_TRN_JOINT = 0, DMC_TRN_TENDON = 3 };
enum { DMC_WRAP_JOINT = 1, DMC_WRAP_SITE = 3 };
enum { DMC_EQ_CONNECT = 0, DMC_EQ_WELD = 1, DMC_EQ_JOINT = 2, DMC_EQ_TENDON = 3 };   /* mjtEq */
enum { DMC_DYN_NONE = 0, DMC_DYN_INTEGRATOR = 1, DMC_DYN_FILTER = 2, DMC_DYN_FILTEREXACT = 3 };
enum { DMC_GAIN_FIXED = 0, DMC_GAIN_AFFINE = 1 };
enum { DMC_BIAS_NONE = 0, DMC_BIAS_AFFINE = 1 };
enum { DMC_OBJ_BODY = 1, DMC_OBJ_XBODY = 2, DMC_OBJ_JOINT = 3, DMC_OBJ_GEOM = 5, DMC_OBJ_SITE = 6, DMC_OBJ_ACTUATOR = 19 };
enum { DMC_STAGE_NONE = 0, DMC_STAGE_POS = 1, DMC_STAGE_VEL = 2, DMC_STAGE_ACC = 3 };
enum { DMC_SENS_TOUCH = 0, DMC_SENS_ACCELEROMETER = 1, DMC_SENS_VELOCIMETER = 2,
       DMC_SENS_GYRO = 3, DMC_SENS_FORCE = 4, DMC_SENS_TORQUE = 5,
       DMC_SENS_JOINTPOS = 9, DMC_SENS_JOINTVEL = 10, DMC_SENS_ACTUATORFRC = 15,
       DMC_SENS_RANGEFINDER = 7,
       DMC_SENS_FRAMEPOS = 26, DMC_SENS_FRAMEQUAT = 27, DMC_SENS_FRAMEXAXIS = 28, DMC_SENS_FRAMEYAXIS = 29, DMC_SENS_FRAMEZAXIS = 30,
       DMC_SENS_FRAMELINVEL = 31, DMC_SENS_FRAMEANGVEL = 32,
       DMC_SENS_SUBTREECOM = 37, DMC_SENS_SUBTREELINVEL = 38 };
/* mjtDisableBit, in the order of dm_control/mjcf/schema.xml:82-103 */
enum { DMC_DSBL_CONSTRAINT = 1 << 0, DMC_DSBL_EQUALITY = 1 << 1,
       DMC_DSBL_FRICTIONLOSS = 1 << 2, DMC_DSBL_LIMIT = 1 << 3,
       DMC_DSBL_CONTACT = 1 << 4, DMC_DSBL_SPRING = 1 << 5,
       DMC_DSBL_DAMPER = 1 << 6, DMC_DSBL_GRAVITY = 1 << 7,
       DMC_DSBL_CLAMPCTRL = 1 << 8, DMC_DSBL_WARMSTART = 1 << 9,
       DMC_DSBL_FILTERPARENT = 1 << 10, DMC_DSBL_ACTUATION = 1 << 11,
       DMC_DSBL_REFSAFE = 1 << 12, DMC_DSBL_SENSOR = 1 << 13,
       DMC_DSBL_MIDPHASE = 1 << 14, DMC_DSBL_EULERDAMP = 1 << 15,
       DMC_DSBL_AUTORESET = 1 << 16,
       /* constraint islands are a DISABLE flag that defaults to enable (mjcf/schema.xml:102) */
       DMC_DSBL_NATIVECCD = 1 << 17, DMC_DSBL_ISLAND = 1 << 18, DMC_DSBL_MULTICCD = 1 << 19 };
enum { DMC_ENBL_OVERRIDE = 1 << 0, DMC_ENBL_ENERGY = 1 << 1 };
/* mjtWarning order as used by Physics.check_invalid_state
 * (dm_control/mujoco/engine.py:345-368) */
enum { DMC_WARN_INERTIA = 0, DMC_WARN_CONTACTFULL = 1, DMC_WARN_CNSTRFULL = 2,
       DMC_WARN_VGEOMFULL = 3, DMC_WARN_BADQPOS = 4, DMC_WARN_BADQVEL = 5,
       DMC_WARN_BADQACC = 6, DMC_WARN_BADCTRL = 7,
       /* not a MuJoCo warning: a geom pair whose shapes the collision kernel cannot
        * resolve (cylinders: tested as their enclosing capsules) came into contact range */
       DMC_WARN_COLLISION = 8, DMC_NWARNING = 9 };

/* ---- the batch's data fields (mjData): X(name, count_expr, flags) --------
 * The one list of what dmc_batch_get / set / bind know by name, in the order of the field ids: the C ABI's field
 * table and its StepIO fill (dmc_api.hip), the host emulation (tests/emu) and dm_control_amd/_layout.py all expand or
 * parse it.  Count expressions are rows per environment over nq nv nu na nbody ngeom nsite nsensordata nmocap nconmax;
 * real fields are stored in the batch precision, int fields as int32.  Flags: */
enum { DMC_FIELD_F64 = 1,     /* stored as fp64 whatever the batch precision */
       DMC_FIELD_ACC_IN = 2,  /* an input of the acceleration stage only: a write leaves the stash epoch alone */
       DMC_FIELD_OPTS = 4 };  /* no StepIO member: reaches the kernel through StepOpts */
#define DMC_DATA_REAL_FIELDS(X) \
  X(qpos, nq, 0) X(qvel, nv, 0) X(ctrl, nu, DMC_FIELD_ACC_IN) X(qacc_warmstart, nv, 0) \
  X(qfrc_applied, nv, DMC_FIELD_ACC_IN) X(xfrc_applied, 6*nbody, DMC_FIELD_ACC_IN | DMC_FIELD_OPTS) \
  X(time, 1, DMC_FIELD_F64) X(act, na, 0) \
  X(mocap_pos, 3*nmocap, DMC_FIELD_OPTS) X(mocap_quat, 4*nmocap, DMC_FIELD_OPTS) \
  X(sensordata, nsensordata, 0) X(xpos, 3*nbody, 0) X(xquat, 4*nbody, 0) X(xmat, 9*nbody, 0) \
  X(xipos, 3*nbody, 0) X(geom_xpos, 3*ngeom, 0) X(geom_xmat, 9*ngeom, 0) \
  X(site_xpos, 3*nsite, 0) X(site_xmat, 9*nsite, 0) X(subtree_com, 3*nbody, 0) \
  X(qacc, nv, 0) X(actuator_force, nu, 0) X(qfrc_actuator, nv, 0) \
  X(qfrc_bias, nv, 0) X(qfrc_constraint, nv, 0) \
  X(contact_dist, nconmax, 0) X(contact_pos, 3*nconmax, 0) X(contact_frame, 9*nconmax, 0) \
  X(contact_force, 6*nconmax, 0) X(cvel, 6*nbody, 0)
#define DMC_DATA_INT_FIELDS(X) \
  X(ncon, 1, 0) X(nefc, 1, 0) X(solver_iter, 1, 0) X(warning, DMC_NWARNING, 0) \
  X(contact_geom1, nconmax, 0) X(contact_geom2, nconmax, 0) X(env_mode, 1, 0)

#define DMC_MINVAL 1e-15
#define DMC_MAXVAL 1e10
#define DMC_MINMU  1e-5
#define DMC_MINIMP 0.0001
#define DMC_MAXIMP 0.9999

#endif  /* DMC_MODEL_LAYOUT_H_ */

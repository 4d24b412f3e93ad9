"""ctypes binding of libdmc_hip.so (include/dmc_batch.h).  There is no CPU
fallback: if the HIP library is missing or fails to load, importing raises."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_VARIANT = 'prof' if os.environ.get('DMC_USE_PROF') else os.environ.get('DMC_LIB_VARIANT')
LIB_PATH = os.path.join(_HERE, 'libdmc_hip_%s.so' % _VARIANT if _VARIANT else 'libdmc_hip.so')

EXPORTS = [
    'dmc_last_error', 'dmc_model_create', 'dmc_model_destroy', 'dmc_batch_create', 'dmc_batch_create_caps',
    'dmc_batch_destroy', 'dmc_batch_step', 'dmc_batch_rollout', 'dmc_batch_forward', 'dmc_batch_reset',
    'dmc_batch_field_rows', 'dmc_batch_get', 'dmc_batch_set', 'dmc_batch_get_int',
    'dmc_batch_set_int', 'dmc_batch_device_ptr', 'dmc_batch_bind',
    'dmc_batch_set_output_mask', 'dmc_batch_set_opt_int', 'dmc_batch_set_opt_real',
    'dmc_batch_set_model_real',
    'dmc_batch_step1', 'dmc_batch_step2', 'dmc_batch_sync', 'dmc_batch_invalidate', 'dmc_batch_invalidate_async', 'dmc_batch_info', 'dmc_batch_time_steps',
    'dmc_batch_enable_profiling', 'dmc_batch_get_timer', 'dmc_batch_set_step_probe', 'dmc_batch_set_async', 'dmc_batch_get_async', 'dmc_batch_get_wait', 'dmc_batch_get_staged',
    'dmc_batch_debug_enable', 'dmc_batch_debug_get', 'dmc_batch_prof_enable',
    'dmc_batch_prof_get', 'dmc_gather_create', 'dmc_gather_destroy', 'dmc_gather_run',
    'dmc_batch_set_env_geoms', 'dmc_env_geom_pack', 'dmc_batch_wave_trace', 'dmc_batch_randomize_joints',
    'dmc_batch_attach_specialised', 'dmc_batch_set_task_args', 'dmc_batch_enable_task',
    'dmc_camera_create', 'dmc_camera_destroy', 'dmc_camera_set_colors', 'dmc_camera_set_materials', 'dmc_camera_set_tuning',
    'dmc_camera_render',
]

# include/dmc_ik.h (batched inverse kinematics: csrc/ik_kernels.hip)
IK_EXPORTS = ['dmc_ik_last_error', 'dmc_ik_create', 'dmc_ik_solve', 'dmc_ik_info', 'dmc_ik_destroy']

# include/dmc_ray.h (batched ray casts: csrc/ray_kernels.hip)
RAY_EXPORTS = ['dmc_rays_create', 'dmc_rays_cast', 'dmc_rays_add_scan', 'dmc_rays_scan', 'dmc_rays_info', 'dmc_rays_destroy']

# include/dmc_dist.h (batched geom distances: csrc/dist_kernels.hip)
DIST_EXPORTS = ['dmc_dist_create', 'dmc_dist_query', 'dmc_dist_info', 'dmc_dist_destroy', 'dmc_geom_distance_host']

# include/dmc_jac.h (batched Jacobians: csrc/jac_kernels.hip)
JAC_EXPORTS = ['dmc_jac_create', 'dmc_jac_jacobian', 'dmc_jac_velocity', 'dmc_jac_force', 'dmc_jac_info', 'dmc_jac_destroy']

# include/dmc_dyn.h (batched dynamics: csrc/dyn_kernels.hip)
DYN_EXPORTS = ['dmc_dyn_create', 'dmc_dyn_mass_matrix', 'dmc_dyn_bias', 'dmc_dyn_inverse', 'dmc_dyn_mul', 'dmc_dyn_solve', 'dmc_dyn_info',
               'dmc_dyn_destroy']

# include/dmc_lin.h (batched linearisation: csrc/lin_kernels.hip)
LIN_EXPORTS = ['dmc_lin_create', 'dmc_lin_transition', 'dmc_lin_fan_out', 'dmc_lin_warnings', 'dmc_lin_info', 'dmc_lin_destroy']

# include/dmc_con.h (batched contact wrenches: csrc/con_kernels.hip)
CON_EXPORTS = ['dmc_con_create', 'dmc_con_wrench', 'dmc_con_net', 'dmc_con_warmstart', 'dmc_con_info', 'dmc_con_destroy']

_lib = None


class NativeError(RuntimeError):
  pass


def lib():
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise NativeError(
        'libdmc_hip.so not built: run `python -m dm_control_amd.build` '
        '(or __graft_entry__.build()).  There is no CPU fallback.')
  # PyTorch-ROCm bundles its own HIP runtime; load it first so that this library
  # and torch share ONE libamdhip64 (two runtimes in a process cannot both see
  # the GPU).  torch is only plumbing here (device memory, streams, RCCL).
  try:
    import torch  # noqa: F401  pylint: disable=unused-import,import-outside-toplevel
  except ImportError:
    pass
  L = ctypes.CDLL(LIB_PATH)
  vp, ci, cd, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_char_p
  L.dmc_last_error.restype = cs
  L.dmc_model_create.argtypes = [vp, ci, vp, ci, ctypes.POINTER(vp)]
  L.dmc_model_destroy.argtypes = [vp]
  L.dmc_batch_create.argtypes = [vp, ci, ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
  L.dmc_batch_destroy.argtypes = [vp]
  L.dmc_batch_step.argtypes = [vp, ci, ci, vp]
  L.dmc_batch_forward.argtypes = [vp, ci, vp]
  L.dmc_batch_rollout.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
  L.dmc_batch_reset.argtypes = [vp, vp, ci]
  L.dmc_batch_field_rows.argtypes = [vp, cs, ctypes.POINTER(ci), ctypes.POINTER(ci)]
  L.dmc_batch_get.argtypes = [vp, cs, vp]
  L.dmc_batch_set.argtypes = [vp, cs, vp]
  L.dmc_batch_get_int.argtypes = [vp, cs, vp]
  L.dmc_batch_set_int.argtypes = [vp, cs, vp]
  L.dmc_batch_device_ptr.restype = vp
  L.dmc_batch_device_ptr.argtypes = [vp, cs]
  L.dmc_batch_bind.argtypes = [vp, cs, vp]
  L.dmc_batch_set_output_mask.argtypes = [vp, ci]
  L.dmc_batch_set_opt_int.argtypes = [vp, cs, ci]
  L.dmc_batch_set_opt_real.argtypes = [vp, cs, cd]
  L.dmc_batch_set_model_real.argtypes = [vp, cs, vp, ci]
  L.dmc_batch_sync.argtypes = [vp]
  L.dmc_batch_invalidate.argtypes = [vp]
  L.dmc_batch_invalidate_async.argtypes = [vp, vp]
  L.dmc_batch_step1.argtypes = [vp, vp]
  L.dmc_batch_create_caps.argtypes = [vp, ci, ci, ci, vp, ci, ctypes.POINTER(vp)]
  L.dmc_batch_set_env_geoms.argtypes = [vp, ci, vp]
  L.dmc_env_geom_pack.argtypes = [ci, vp, vp, vp, vp]
  L.dmc_gather_create.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_char_p), vp, vp, vp, ctypes.POINTER(vp)]
  L.dmc_gather_destroy.argtypes = [vp]
  L.dmc_gather_destroy.restype = None
  L.dmc_gather_run.argtypes = [vp, vp, vp]
  L.dmc_batch_step2.argtypes = [vp, vp]
  L.dmc_batch_info.argtypes = [vp, vp]
  L.dmc_batch_time_steps.argtypes = [vp, ci, ci, ci, vp, ctypes.POINTER(ctypes.c_float)]
  L.dmc_batch_enable_profiling.argtypes = [vp, ci]
  L.dmc_batch_set_step_probe.argtypes = [vp, ci, vp, ci]
  L.dmc_batch_set_async.argtypes = [vp, cs, vp, ci, vp]
  L.dmc_batch_get_async.argtypes = [vp, ci, ctypes.POINTER(cs), vp]
  L.dmc_batch_get_wait.argtypes = [vp, ci, ctypes.POINTER(vp), ci]
  L.dmc_batch_get_staged.argtypes = [vp, ci]
  L.dmc_batch_get_staged.restype = vp
  L.dmc_batch_get_timer.argtypes = [vp, ci, ctypes.POINTER(cd), ctypes.POINTER(ctypes.c_longlong)]
  L.dmc_batch_debug_enable.argtypes = [vp, ci]
  L.dmc_batch_debug_get.argtypes = [vp, cs, ci, vp, ctypes.POINTER(ci)]
  L.dmc_batch_prof_enable.argtypes = [vp, ci]
  L.dmc_batch_prof_get.argtypes = [vp, vp, ctypes.POINTER(ci)]
  L.dmc_batch_wave_trace.argtypes = [vp, ci, vp, ctypes.POINTER(ci)]
  L.dmc_batch_randomize_joints.argtypes = [vp, ctypes.c_uint64, vp, vp, ci, vp]
  if hasattr(L, 'dmc_batch_attach_specialised'):      # (absent from the older libraries A/B runs load as variants)
    L.dmc_batch_attach_specialised.argtypes = [vp, cs]
  if hasattr(L, 'dmc_batch_set_task_args'):
    L.dmc_batch_set_task_args.argtypes = [vp, vp, ci]
    L.dmc_batch_enable_task.argtypes = [vp, ci]
  if hasattr(L, 'dmc_camera_create'):
    L.dmc_camera_create.argtypes = [vp, ci, vp, ci, ci, vp, ctypes.POINTER(vp)]
    L.dmc_camera_destroy.argtypes = [vp]
    L.dmc_camera_destroy.restype = None
    L.dmc_camera_set_colors.argtypes = [vp, vp, vp]
    if hasattr(L, 'dmc_camera_set_materials'):      # (absent from a library variant built before the textures: A/B timing)
      L.dmc_camera_set_materials.argtypes = [vp, vp, vp, ci]
    L.dmc_camera_set_tuning.argtypes = [vp, ci, ci]
    L.dmc_camera_render.argtypes = [vp, ci, vp, vp, vp, vp]
  if hasattr(L, 'dmc_ik_create'):      # (absent from the older libraries A/B runs load as variants)
    L.dmc_ik_last_error.restype = cs
    L.dmc_ik_create.argtypes = [vp, vp, vp, ctypes.POINTER(vp)]
    L.dmc_ik_solve.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.dmc_ik_info.argtypes = [vp, vp]
    L.dmc_ik_destroy.argtypes = [vp]
    L.dmc_ik_destroy.restype = None
  if hasattr(L, 'dmc_rays_create'):      # (absent from the older libraries A/B runs load as variants)
    L.dmc_rays_create.argtypes = [vp, vp, ctypes.POINTER(vp)]
    L.dmc_rays_cast.argtypes = [vp, ci, vp, vp, ci, vp, ci, vp, vp, vp, vp]
    L.dmc_rays_add_scan.argtypes = [vp, ci, ci, vp, ci, ci, vp]
    L.dmc_rays_scan.argtypes = [vp, vp, vp, vp, vp]
    L.dmc_rays_info.argtypes = [vp, vp]
    L.dmc_rays_destroy.argtypes = [vp]
    L.dmc_rays_destroy.restype = None
  if hasattr(L, 'dmc_dist_create'):      # (absent from the older libraries A/B runs load as variants)
    L.dmc_dist_create.argtypes = [vp, ci, vp, vp, ci, vp, vp, ctypes.POINTER(vp)]
    L.dmc_dist_query.argtypes = [vp, vp, vp, vp, vp, vp]
    L.dmc_dist_info.argtypes = [vp, vp]
    L.dmc_dist_destroy.argtypes = [vp]
    L.dmc_dist_destroy.restype = None
    L.dmc_geom_distance_host.argtypes = [ci, vp, vp, vp, ci, vp, vp, vp, cd, cd, ci, vp, vp]
    L.dmc_geom_distance_host.restype = cd
  if hasattr(L, 'dmc_jac_create'):
    i64 = ctypes.c_int64
    L.dmc_jac_create.argtypes = [vp, vp, ctypes.POINTER(vp)]
    L.dmc_jac_jacobian.argtypes = [vp, vp, vp, vp, vp]
    L.dmc_jac_velocity.argtypes = [vp, ci, vp, vp]
    L.dmc_jac_force.argtypes = [vp, vp, i64, i64, vp, i64, i64, vp, vp]
    L.dmc_jac_info.argtypes = [vp, vp]
    L.dmc_jac_destroy.argtypes = [vp]
    L.dmc_jac_destroy.restype = None
  if hasattr(L, 'dmc_dyn_create'):
    i64 = ctypes.c_int64
    L.dmc_dyn_create.argtypes = [vp, vp, ci, ctypes.POINTER(vp)]
    L.dmc_dyn_mass_matrix.argtypes = [vp, vp, vp]
    L.dmc_dyn_bias.argtypes = [vp, vp, vp]
    L.dmc_dyn_inverse.argtypes = [vp, vp, i64, vp, vp]
    L.dmc_dyn_mul.argtypes = [vp, vp, ci, vp, vp]
    L.dmc_dyn_solve.argtypes = [vp, vp, ci, vp, vp]
    L.dmc_dyn_info.argtypes = [vp, vp]
    L.dmc_dyn_destroy.argtypes = [vp]
    L.dmc_dyn_destroy.restype = None
  if hasattr(L, 'dmc_lin_create'):
    L.dmc_lin_create.argtypes = [vp, vp, vp, cd, ci, ci, ctypes.POINTER(vp)]
    L.dmc_lin_transition.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
    L.dmc_lin_fan_out.argtypes = [vp, ci, ci, vp]
    L.dmc_lin_warnings.argtypes = [vp, vp, vp]
    L.dmc_lin_info.argtypes = [vp, vp]
    L.dmc_lin_destroy.argtypes = [vp]
    L.dmc_lin_destroy.restype = None
  if hasattr(L, 'dmc_con_create'):
    L.dmc_con_create.argtypes = [vp, vp, ctypes.POINTER(vp)]
    L.dmc_con_wrench.argtypes = [vp, vp, vp]
    L.dmc_con_net.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    L.dmc_con_warmstart.argtypes = [vp, ci, vp]
    L.dmc_con_info.argtypes = [vp, vp]
    L.dmc_con_destroy.argtypes = [vp]
    L.dmc_con_destroy.restype = None
  _lib = L
  return L


def check(rc):
  if rc != 0:
    raise NativeError(lib().dmc_last_error().decode() or ('error %d' % rc))

"""Builds libdmc_hip.so (HIP kernels + C-ABI) in-tree for gfx950 with hipcc.

hipcc cross-compiles without a GPU.  The library is git-ignored but travels to
the GPU box with the working-tree snapshot.
"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libdmc_hip.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ARCH = 'gfx950'

_COMMON = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function', '-Wno-missing-braces']
# Every file the step kernels are built from, relative to csrc/: what a step unit includes, and the host side that decides
# the layout baked into them (step_tables.h) and the C ABI (dmc_batch.h).  The one list: the staleness check below, the key
# of the plugin cache (specialise.py) and the host build of the tests (tests/emu_lib.py) all read it, and
# tests/test_core_headers_cpu.py holds it against the #include lines.
STEP_SOURCES = ('step_kernel.hip.h', 'step_core.h', 'step_defs.h', 'step_math.h', 'step_lanes.h', 'step_dense.h',
                'step_geom.h', 'step_layout.h', 'step_tables.h',
                '../../include/dmc_model_layout.h', '../../include/dmc_batch.h')
_UNITS = [
    # default fp contraction (fma); fp32 division / square root as the 2.5-ulp hardware forms and fp32 denormals
    # flushed (config 2 +2.6 %, config 4 +2.9 %, A/B on one box; the fp32 parity tolerances are unchanged)
    ('step_kernels_f32.hip', ['-fno-hip-fp32-correctly-rounded-divide-sqrt', '-fgpu-flush-denormals-to-zero']),
    # the fp32 instantiations of the LARGE models (_STATIC_MODELS entries marked 'ilp') as their own unit, scheduled
    # for instruction-level parallelism instead of the default occupancy-driven strategy: these kernels sit at the
    # 256-VGPR cap anyway and run one or two latency-bound waves per SIMD (A/B of the whole library built this way,
    # one box: config 4 +7.5 %, config 5 +3.9 %, config 3 -0.6 %, config 2 -3.1 % -- hence only the large ones)
    ('step_kernels_f32_ilp.hip', ['-fno-hip-fp32-correctly-rounded-divide-sqrt', '-fgpu-flush-denormals-to-zero',
                                  '-mllvm', '-amdgpu-sched-strategy=max-ilp']),
    ('step_kernels_f64.hip', ['-ffp-contract=off']),    # rounds like the fp64 oracle
    # batched ray-cast cameras (fp32 and fp64 instantiations); a third entry lists a unit's own headers
    ('camera_kernels.hip', [], ['camera_core.h', '../../include/dmc_model_layout.h']),
    # batched inverse kinematics (fp32 and fp64, position / rotation / both targets), kernel and host entry points;
    # no contraction: the fp64 instantiation rounds like the host build the tests compare it with
    ('ik_kernels.hip', ['-ffp-contract=off'], ['ik_core.h', 'step_defs.h', 'step_math.h', '../../include/dmc_model_layout.h',
                                               '../../include/dmc_ik.h', '../../include/dmc_batch.h']),
    # batched ray casts (fp32 and fp64: arbitrary rays, scans in a moving frame); the closed forms are the camera's
    ('ray_kernels.hip', [], ['ray_core.h', 'camera_core.h', '../../include/dmc_model_layout.h']),
    # batched geom distances (fp32 and fp64: GJK + EPA per (environment, pair)); no contraction: the fp64 instantiation
    # rounds like the host build of the same header (dmc_geom_distance_host, the tests' emulation)
    ('dist_kernels.hip', ['-ffp-contract=off'], ['dist_core.h', '../../include/dmc_model_layout.h']),
    # batched Jacobians (fp32 and fp64: mj_jac, J qvel, J' f per (environment, target)); no contraction: the fp64
    # instantiation rounds like the host build of the same header (the tests' emulation)
    ('jac_kernels.hip', ['-ffp-contract=off'], ['jac_core.h', 'step_defs.h', 'step_math.h', '../../include/dmc_model_layout.h']),
    # batched dynamics (fp32 and fp64: mj_fullM, mj_mulM, mj_solveM, mj_rne per environment); no contraction: the fp64
    # instantiation rounds like the host build of the same header (the tests' emulation)
    ('dyn_kernels.hip', ['-ffp-contract=off'], ['dyn_core.h', 'jac_core.h', 'step_defs.h', 'step_math.h', '../../include/dmc_model_layout.h']),
    # batched linearisation (mjd_transitionFD per environment: the fan-out into perturbed columns and their differencing,
    # for the precision pairs fp64/fp64, fp32 source/fp64 scratch, fp32/fp32); no contraction: the fp64 instantiation
    # rounds like the host build of the same header (the tests' emulation)
    ('lin_kernels.hip', ['-ffp-contract=off'], ['lin_core.h', 'step_defs.h', 'step_math.h', '../../include/dmc_model_layout.h']),
    # batched contact wrenches (fp32 and fp64: the world wrench per contact slot, the net wrench per (environment, target));
    # no contraction: the fp64 instantiation rounds like the host build of the same header (the tests' emulation)
    ('con_kernels.hip', ['-ffp-contract=off'], ['con_core.h', 'step_defs.h', '../../include/dmc_model_layout.h']),
    # (the ray, distance, Jacobian, dynamics, linearisation and contact entry points' headers -- ray_core.h, dmc_ray.h,
    # dist_core.h, dmc_dist.h, jac_core.h, dmc_jac.h, dyn_core.h, dmc_dyn.h, lin_core.h, dmc_lin.h, con_core.h, dmc_con.h --
    # reach the staleness check through _own_includes)
    ('dmc_api.hip', [], list(STEP_SOURCES) + ['camera_core.h']),
]


def _stale(target, sources):
  if not os.path.exists(target):
    return True
  t = os.path.getmtime(target)
  return any(os.path.getmtime(s) > t for s in sources)


def _own_includes(src):
  """The files a unit's own text includes with quotes, followed through their includes in turn, where they exist: a unit
  is stale against them whether or not its _UNITS entry lists them.  Generated headers (*.gen.h) are left out: build()
  names the one its build variant uses, and a production unit is not stale against the profiling layouts."""
  found, todo = [], [src]
  while todo:
    path = todo.pop()
    with open(path) as f:
      names = re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
    for p in (os.path.normpath(os.path.join(os.path.dirname(path), n)) for n in names):
      if p != src and p not in found and not p.endswith('.gen.h') and os.path.exists(p):
        found.append(p)
        todo.append(p)
  return found


# suite models that get model-specialised kernel instantiations: (asset, [lanes...], (nconmax, njmax[, njcon])); the caps
# must be the ones the suite uses (suite/common.py DEFAULT_CAPS), 0 = the library default
_STATIC_MODELS = [('cheetah', [32, 16], (0, 0)), ('humanoid', [64], (24, 0)), ('cartpole', [32], (0, 0)),
                  ('walker', [32], (0, 0)), ('hopper', [32], (0, 0)),
                  ('humanoid_CMU', [64], (96, 0), 'ilp'), ('cmu_2019_position_floor', [64], (48, 0), 'ilp'),
                  ('soccer_2v2_boxhead', [64], (24, 0), 'ilp'),
                  # the same model for a batch of at most one environment per CU: everything in LDS (caps: nconmax, njmax, njcon, jglobal + 1)
                  ('soccer_2v2_boxhead', [64], (24, 0, 0, 1), 'ilp')]
GEN = os.path.join(CSRC, 'static_layouts.gen.h')
GEN_PROF = os.path.join(CSRC, 'static_layouts_prof.gen.h')


def generate_static_layouts(verbose=False, profile=False):
  """Bakes the LDS layouts of the suite models into csrc/static_layouts.gen.h (profiling builds: the layouts with
  the phase counters in them, into static_layouts_prof.gen.h, so that they run the model-specialised kernels too)."""
  import tempfile
  sys.path.insert(0, os.path.dirname(HERE))
  from dm_control_amd import mjcf_compiler
  tool = os.path.join(CSRC, 'gen_static_layouts' + ('_prof' if profile else ''))
  src = os.path.join(CSRC, 'gen_static_layouts.cpp')
  GEN = GEN_PROF if profile else globals()['GEN']
  deps = [src] + [os.path.join(CSRC, d) for d in ('step_tables.h', 'step_layout.h', '../../include/dmc_model_layout.h')]
  if _stale(tool, deps):
    subprocess.check_call(['g++', '-O1', '-std=c++17'] + (['-DDMC_PROFILE=1'] if profile else []) + ['-o', tool, src])
  lines = ['// GENERATED by dm_control_amd/build.py -- do not edit', '#pragma once']
  inits, inst, inst_ilp = [], [], []
  for sid, (name, lanes, caps, *unit) in enumerate(_STATIC_MODELS):
    with open(os.path.join(HERE, 'suite', 'assets', name + '.xml')) as f:
      m = mjcf_compiler.compile_xml(f.read())
    ints, reals = m.pack()
    with tempfile.TemporaryDirectory() as td:
      fi, fr = os.path.join(td, 'i.bin'), os.path.join(td, 'r.bin')
      ints.tofile(fi)
      reals.tofile(fr)
      init = subprocess.check_output([tool, name, fi, fr] + [str(c) for c in caps]).decode().strip()
    lines.append('#define DMC_STATIC_LAYOUT_%d %s  // %s' % (sid, init, name))
    lines.append('#define DMC_STATIC_NV_%d %d' % (sid, m.nv))
    inits.append('DMC_STATIC_LAYOUT_%d' % sid)
    (inst_ilp if unit else inst).extend('X(%d, %d)' % (sid, l) for l in lanes)
  lines.append('#define DMC_NSTATIC %d' % len(_STATIC_MODELS))
  lines.append('#define DMC_STATIC_LAYOUT_LIST {%s}' % ', '.join(inits))
  lines.append('#define DMC_STATIC_INSTANCES(X) %s' % ' '.join(inst + inst_ilp))
  lines.append('#define DMC_STATIC_INSTANCES_STD(X) %s' % ' '.join(inst))       # fp32: step_kernels_f32.hip
  lines.append('#define DMC_STATIC_INSTANCES_ILP(X) %s' % ' '.join(inst_ilp))   # fp32: step_kernels_f32_ilp.hip
  lines.append('#define DMC_STATIC_IDS(X) %s' % ' '.join('X(%d)' % k for k in range(len(_STATIC_MODELS))))
  text = '\n'.join(lines) + '\n'
  old = open(GEN).read() if os.path.exists(GEN) else None
  if old != text:
    with open(GEN, 'w') as f:
      f.write(text)
    if verbose:
      print('wrote', GEN, file=sys.stderr)


def build(force=False, verbose=False, profile=False, variant=None, extra_flags=()):
  """profile=True builds libdmc_hip_prof.so with per-phase cycle counters
  (-DDMC_PROFILE) next to the production library.  variant/extra_flags build an
  experimental libdmc_hip_<variant>.so (tuning studies; select it at run time
  with DMC_LIB_VARIANT=<variant>)."""
  generate_static_layouts(verbose, profile)
  deps = [os.path.join(CSRC, d) for d in STEP_SOURCES] + [GEN_PROF if profile else GEN]
  objs = []
  procs = []
  tag = 'prof' if profile else variant
  lib = LIB.replace('.so', '_%s.so' % tag) if tag else LIB
  for src, flags, *own in _UNITS:
    s = os.path.join(CSRC, src)
    udeps = [os.path.join(CSRC, d) for d in own[0]] + deps[-1:] if own else deps
    o = os.path.join(CSRC, src.replace('.hip', '_%s.o' % tag if tag else '.o'))
    flags = flags + list(extra_flags)
    if profile:
      flags = flags + ['-DDMC_PROFILE=1']
    objs.append(o)
    if force or _stale(o, [s] + udeps + _own_includes(s)):
      cmd = [HIPCC] + _COMMON + flags + ['-c', s, '-o', o]
      if verbose:
        print(' '.join(cmd), file=sys.stderr)
      procs.append((cmd, subprocess.Popen(cmd)))
  for cmd, p in procs:
    if p.wait() != 0:
      raise RuntimeError('hipcc failed: ' + ' '.join(cmd))
  if force or procs or _stale(lib, objs):
    cmd = [HIPCC, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-o', lib] + objs
    if verbose:
      print(' '.join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
  return lib


if __name__ == '__main__':
  var = [a.split('=', 1)[1] for a in sys.argv if a.startswith('--variant=')]
  xf = [a for a in sys.argv if a.startswith(('-D', '-m', '-f'))]
  print(build(force='--force' in sys.argv, verbose=True, profile='--profile' in sys.argv,
              variant=var[0] if var else None, extra_flags=xf))

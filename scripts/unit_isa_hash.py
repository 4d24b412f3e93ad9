"""Device assembly of every kernel unit of one source tree, hashed: the check that a refactor changes no instruction.
   python scripts/unit_isa_hash.py <tree> <outdir>      -- prints {unit: sha256} as JSON; the .s files stay in <outdir>
Units: the three step units of the library and its add-on units camera_kernels, ray_kernels and ik_kernels (each with
its own flags of build.py, plus --cuda-device-only -S) and step_kernel_spec.hip for the cheetah at fp32 and fp64, the
command being the one specialise.build issues with `-shared -o <plugin>` replaced.  Lines that hold the per-compilation
`__hip_cuid_<hash>` symbol are dropped before hashing;
two trees changed no kernel iff all eight hashes agree.  No GPU is needed; about 15 CPU-minutes per tree."""
import hashlib, json, os, subprocess, sys, tempfile
tree, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
os.makedirs(out, exist_ok=True)
sys.path.insert(0, tree)
from dm_control_amd import build as B, specialise as S, mjcf_compiler
assert os.path.dirname(B.HERE) == tree, 'dm_control_amd was imported from %s' % B.HERE
B.generate_static_layouts()
procs = []
for src, flags, *_ in B._UNITS:
  if src != 'dmc_api.hip':      # (the host side: no kernel of its own)
    cmd = [B.HIPCC] + B._COMMON + flags + ['--cuda-device-only', '-S', os.path.join(B.CSRC, src), '-o', os.path.join(out, src.replace('.hip', '.s'))]
    procs.append((src.replace('.hip', ''), subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
os.environ['DMC_SPEC_CACHE'] = tempfile.mkdtemp()
os.environ.pop('DMC_SPEC_FLAGS', None)
with open(os.path.join(B.HERE, 'suite', 'assets', 'cheetah.xml')) as f:
  model = mjcf_compiler.compile_xml(f.read())
check_call = subprocess.check_call
names = [n for n, _ in procs]
for prec in (32, 64):
  name = 'spec_cheetah_f%d' % prec
  names.append(name)
  def to_assembly(cmd, name=name, **kw):
    if '-shared' not in cmd:
      return check_call(cmd, **kw)
    i = cmd.index('-shared')      # [..., '-shared', '-o', <plugin>, <source>]
    check_call(cmd[:i] + ['--cuda-device-only', '-S', '-o', os.path.join(out, name + '.s')] + cmd[i + 3:], stderr=subprocess.DEVNULL, **kw)
    open(cmd[i + 2], 'w').close()
  S.subprocess.check_call = to_assembly
  S.build(model, precision=prec)
S.subprocess.check_call = check_call
for n, p in procs:
  if p.wait() != 0:
    sys.exit('hipcc failed on ' + n)
res = {}
for n in names:
  with open(os.path.join(out, n + '.s'), 'rb') as f:
    res[n] = hashlib.sha256(b'\n'.join(l for l in f.read().split(b'\n') if b'__hip_cuid_' not in l)).hexdigest()
print(json.dumps(res, indent=1))

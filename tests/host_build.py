"""TEST INFRASTRUCTURE: the one host build of the tests' C++ (tests/emu/*.cpp, each a host form of device code)."""
import ctypes
import fcntl
import os
import subprocess

from dm_control_amd import build


def load(src, name, flags=(), opt='-O2', out_dir=None, deps=()):
  """lib<name>.so next to `src` (or in out_dir), rebuilt when older than src, anything it includes (followed through the
  quoted includes) or `deps`, and loaded.  pytest-xdist workers may all find it stale at once: one builds under a lock, into
  a temporary that is moved in place atomically -- a worker never loads a half-written object."""
  so = os.path.join(out_dir or os.path.dirname(src), 'lib%s.so' % name)
  sources = [src] + build._own_includes(src) + list(deps)      # pylint: disable=protected-access
  stale = lambda: not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in sources)
  if stale():
    with open(so + '.lock', 'w') as lk:
      fcntl.flock(lk, fcntl.LOCK_EX)
      if stale():
        tmp = so + '.%d.tmp' % os.getpid()
        subprocess.check_call(['g++', opt, '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas'] +
                              list(flags) + ['-o', tmp, src])
        os.replace(tmp, so)
  return ctypes.CDLL(so)

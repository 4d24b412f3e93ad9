"""The headers the step core is split into (dm_control_amd/csrc/step_{defs,math,lanes,dense,geom}.h) and the one list of
the step kernels' sources (dm_control_amd/build.py STEP_SOURCES: build staleness, the key of the plugin cache, the host
build of the tests)."""
import os
import subprocess

import pytest

from dm_control_amd import build, specialise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('step_defs.h', 'step_math.h', 'step_lanes.h', 'step_dense.h', 'step_geom.h')


@pytest.mark.parametrize('header', HEADERS)
def test_header_is_self_contained(header, tmp_path):
  """Each compiles as a translation unit of its own (host form): in particular step_geom.h needs nothing of the core, so
  that other code -- tests/emu/geom_emu.cpp -- can share the narrow phase and the rays."""
  tu = tmp_path / 'tu.cpp'
  tu.write_text('#include "%s"\n' % os.path.join(build.CSRC, header))
  subprocess.check_call(['g++', '-std=c++17', '-fsyntax-only', '-DDMC_HOST_EMU', str(tu)])


def _reach(roots):
  """What the roots include, followed through (build._own_includes); generated headers are not sources."""
  roots = [os.path.join(build.CSRC, r) for r in roots]
  return {p for r in roots for p in build._own_includes(r) if not p.endswith('.gen.h')} - set(roots)      # pylint: disable=protected-access


def test_source_list_is_complete():
  """What the step kernels' units include, followed through csrc/ and include/, IS the list -- a header added to the core
  and not listed would leave the plugin cache serving kernels built from old sources.  Files of the list that only
  the host units include (the layout tables, the C ABI) are left out of the comparison, but must be included there."""
  listed = {os.path.normpath(os.path.join(build.CSRC, f)) for f in build.STEP_SOURCES}
  assert len(listed) == len(build.STEP_SOURCES)
  kernel = _reach(['step_kernel_spec.hip', 'step_kernels_f32.hip'])
  assert all(p.startswith((build.CSRC, os.path.join(ROOT, 'include'))) for p in kernel)
  assert not kernel - listed, 'included by the step kernels, missing in build.STEP_SOURCES: %s' % sorted(kernel - listed)
  host_only = listed - kernel
  assert {os.path.basename(p) for p in host_only} == {'step_tables.h', 'dmc_batch.h'}
  assert host_only <= _reach(['dmc_api.hip', 'gen_static_layouts.cpp'])


def test_consumers_derive_from_the_list():
  assert set(specialise._SOURCES) == set(build.STEP_SOURCES) | {'step_kernel_spec.hip'}      # pylint: disable=protected-access
  units = {u[0]: u for u in build._UNITS}      # pylint: disable=protected-access
  assert set(units['dmc_api.hip'][2]) == set(build.STEP_SOURCES) | {'camera_core.h'}
  for h in HEADERS + ('step_core.h',):
    assert h in build.STEP_SOURCES


def test_own_includes_follow_the_headers_headers():
  """ray_kernels.hip reaches camera_core.h through ray_core.h alone: the staleness checks of the library build and of the
  tests' host builds (tests/host_build.py) see a header however deep it is included."""
  src = os.path.join(build.CSRC, 'ray_kernels.hip')
  with open(src) as f:
    assert '"camera_core.h"' not in f.read()
  assert os.path.join(build.CSRC, 'camera_core.h') in build._own_includes(src)      # pylint: disable=protected-access

"""The record of the kinematic stash (kstash_record, csrc/step_layout.h: one definition for the kernels that move it in
16-byte pieces and for the allocation) over every suite asset, in both precisions.  No GPU.

The stride is at least the packed record (nq + nv + n_kin) the -DDMC_NO_WIDE_IO kernels and the host build keep, and a
multiple of 16 bytes; the kinematic range starts behind (qpos, qvel) at the phase its LDS copy has against a 16-byte
boundary, so a piece of the record and the piece of the scratch it mirrors are aligned together; one record ends
within the nq + nv + n_kin + 4 elements the host build of the kernel core gives its single environment.  The kernels
also rely on every table and scratch count being a multiple of four elements (tables copied as one list of 16-byte
chunks, an environment's scratch on a 16-byte boundary of LDS): held here against step_layout_build."""
import ctypes
import glob
import os

import numpy as np
import pytest

import host_build
from dm_control_amd import mjcf_compiler as mc
from dm_control_amd.suite import common

HERE = os.path.dirname(os.path.abspath(__file__))
ASSETS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, '..', 'dm_control_amd', 'suite', 'assets', '*.xml')))


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
  L = host_build.load(os.path.join(HERE, 'emu', 'kstash_record.cpp'), 'kstash_record', opt='-O1',
                      out_dir=str(tmp_path_factory.mktemp('kstash_record')))
  L.kstash_facts.restype = ctypes.c_int
  return L


@pytest.mark.parametrize('name', ASSETS)
def test_record_of_every_suite_asset(lib, name):
  m = mc.compile_xml(common.read_model(name + '.xml'))
  ints, reals = m.pack()
  ints = np.ascontiguousarray(ints, dtype=np.int32)
  reals = np.ascontiguousarray(reals, dtype=np.float64)
  out = np.zeros(13, dtype=np.int32)
  nconmax = int(common.DEFAULT_CAPS.get(name, {}).get('nconmax', 0))
  rc = lib.kstash_facts(ctypes.c_void_p(ints.ctypes.data), int(ints.size), ctypes.c_void_p(reals.ctypes.data), int(reals.size),
                        nconmax, ctypes.c_void_p(out.ctypes.data))
  assert rc == 0
  nq, nv, s_xpos, s_qM, n_mi, n_mr_lds, n_mc, n_sr, n_si = (int(x) for x in out[:9])
  assert (nq, nv) == (m.nq, m.nv)
  nk = s_qM - s_xpos
  assert nk > 0
  for p, elem in enumerate((4, 8)):
    kin, stride = int(out[9 + 2*p]), int(out[10 + 2*p])
    per = 16 // elem
    assert stride >= nq + nv + nk                      # at least the packed record
    assert (stride * elem) % 16 == 0                   # whole 16-byte pieces from one record to the next
    assert kin >= nq + nv and kin + nk <= stride       # the range lies behind (qpos, qvel), inside the record
    assert (kin - s_xpos) % per == 0                   # ... at the phase of its LDS copy: pieces aligned on both sides
    assert kin + nk <= nq + nv + nk + 4                # one record fits what the host build allocates
    assert kin - (nq + nv) < per                       # (the gap is less than one piece)
  for cnt in (n_mi, n_mr_lds, n_mc, n_sr, n_si):
    assert cnt % 4 == 0

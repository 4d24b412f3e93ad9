"""The batch's data fields exist once, in include/dmc_model_layout.h (DMC_DATA_REAL_FIELDS / DMC_DATA_INT_FIELDS): what
dm_control_amd/_layout.py parses from it agrees with what the C side expands from it, and the oracle stand-in of the CPU
tier takes its rows from the same list."""
import os

import pytest

import data_fields_model
from dm_control_amd import _layout, mjcf_compiler as mc
from emu_lib import EmuPhysics
from oracle_backend import OracleBatch

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dm_control_amd', 'suite', 'assets')


def _cheetah():
  with open(os.path.join(ASSETS, 'cheetah.xml')) as f:
    return mc.compile_xml(f.read())


MODELS = {'cheetah': (_cheetah, 0), 'small': (data_fields_model.model, data_fields_model.NCONMAX)}


def test_parsed_lists_are_non_empty_and_without_duplicates():
  names = [n for n, _ in _layout.DATA_REAL_FIELDS + _layout.DATA_INT_FIELDS]
  assert _layout.DATA_REAL_FIELDS and _layout.DATA_INT_FIELDS
  assert len(set(names)) == len(names)
  assert {'qpos', 'time', 'xfrc_applied', 'mocap_quat', 'contact_frame', 'cvel'} <= {n for n, _ in _layout.DATA_REAL_FIELDS}
  assert {'ncon', 'warning', 'env_mode'} <= {n for n, _ in _layout.DATA_INT_FIELDS}


@pytest.mark.parametrize('name', sorted(MODELS))
def test_evaluated_rows_equal_the_emulation_and_cover_the_oracle_backend(name):
  make, nconmax = MODELS[name]
  m = make()
  if name == 'small':
    assert m.nmocap > 0 and m.na > 0
  emu = EmuPhysics(m, nconmax=nconmax)
  counts = _layout.data_field_counts(m, emu.nconmax)
  assert counts == emu.field_rows()
  assert counts['qpos'] == m.nq and counts['mocap_quat'] == 4 * m.nmocap and counts['act'] == m.na
  assert counts['contact_frame'] == 9 * emu.nconmax and counts['warning'] == 9
  ob = OracleBatch(m, 1, nconmax=emu.nconmax)
  assert ob._rows and all(counts[n] == r for n, r in ob._rows.items())

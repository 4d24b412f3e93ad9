"""suite/task_arrays.py: the numpy surface the task ports may rely on is the one both array backends serve."""
import os
import subprocess
import sys

import numpy as np

from dm_control_amd.suite import device_env, fused_env, task_arrays


def test_both_backends_serve_the_declared_surface_and_the_gap_is_the_recorded_one():
  device_env._ensure_tables()
  common = set(task_arrays.PORT_FUNCTIONS)
  assert len(common) == len(task_arrays.PORT_FUNCTIONS)
  for cls, funcs in ((device_env.TArr, device_env._FUNCS), (fused_env.SArr, fused_env._FUNCS)):
    only = task_arrays.ONE_BACKEND_ONLY[cls.__name__]
    assert issubclass(cls, task_arrays.TaskArray) and cls._FUNCS is funcs
    assert set(funcs) == common | {f for f in only if not isinstance(f, str)}
    for m in task_arrays.PORT_METHODS + tuple(f for f in only if isinstance(f, str)):
      assert callable(getattr(cls, m))
  assert not hasattr(device_env.TArr, 'flatten')
  assert set(device_env._UFUNCS) == set(task_arrays.PORT_UFUNCS)
  g = fused_env.Graph()
  fused_env._G = g
  try:
    x = fused_env.SArr(np.array([g.load('qpos', 0), g.load('qpos', 1)], dtype=object))
    for name in task_arrays.PORT_UFUNCS:
      uf = getattr(np, name)
      assert isinstance(uf(*([x] * uf.nin)), fused_env.SArr), name
  finally:
    fused_env._G = None


def test_operators_are_plain_functions_of_the_base_class():
  for name in list(task_arrays._BINARY_OPERATORS) + list(task_arrays._UNARY_OPERATORS):
    assert name in vars(task_arrays.TaskArray) and name not in vars(device_env.TArr) and name not in vars(fused_env.SArr)
  assert task_arrays.TaskArray.__hash__ is None and not hasattr(task_arrays.TaskArray, '__getattr__')


def test_the_task_ports_import_without_torch():
  code = "import sys, dm_control_amd.suite.common, dm_control_amd.suite.task_arrays; assert 'torch' not in sys.modules"
  subprocess.check_call([sys.executable, '-c', code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

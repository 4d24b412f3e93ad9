"""The fused passes of the line search's bracket phase (step_core.h primal_search, ls_eval_multi) on the device against
the sequential search they replace: the same sources built with -DDMC_NO_LS_FUSED as an on-demand plugin
(dm_control_amd/specialise.py), against the default kernel.

The fused search evaluates the same points and takes the same decisions; on the register-resident rows of the small
models it also spells out the contraction of an evaluation (ls_terms_regs, ls_point_regs) as the sequential text
compiles, so the two kernels must agree bit for bit -- qpos, qvel, qacc_warmstart, solver_iter, sensordata -- over 240
steps of a seeded batch of 128 environments: cheetah, walker and hopper in fp32 with the library's default (register)
solve, in fp64 with -DDMC_NEWTON_REGS_F64_NV=16 on both sides (the fp64 kernels of the library keep the LDS solve, see
tests/test_gpu_newton_regs.py), one case under a cap of ls_iterations = 4, and the 6-dof chain of
tests/test_gpu_newton_regs.py, whose environments cross the 16 rows of the register solve inside a wave: an environment of
it is compared for as long as every one of its solves had at most 16 rows (past that it runs the LDS text in both builds,
two compilations whose fp32 contraction is the compiler's: DESIGN.md section 4)."""
import numpy as np
import pytest

import test_gpu_newton_regs as nr

pytestmark = pytest.mark.gpu

SEQ_FLAGS = '-DDMC_NO_LS_FUSED'
FIELDS = ('qpos', 'qvel', 'qacc_warmstart', 'solver_iter', 'sensordata')
B, T = 128, 240


def _compare(monkeypatch, name, precision, fused, seq, cap=None, rows_cap=None):
  m = fused.model
  q = nr._init(m, name, B, 1)
  rs = np.random.RandomState(2)
  for b in (fused, seq):
    b.set('qpos', q)
    if cap is not None:
      b.set_opt('ls_iterations', cap)
  clean = np.ones(B, bool)
  first, solves, iters, over = None, 0, 0, 0
  for t in range(T):
    a = rs.uniform(-1, 1, (B, m.nu))
    for b in (fused, seq):
      b.set_control(a)
      b.step()
    n = fused.get('nefc')[:, 0]
    if rows_cap is not None:
      clean &= (n <= rows_cap) & (seq.get('nefc')[:, 0] <= rows_cap)
      over += int((n > rows_cap).sum())
    solves += int(((n > 0) & clean).sum())
    iters += int(fused.get('solver_iter')[clean].sum())
    if first is None and not all(np.array_equal(fused.get(f)[clean], seq.get(f)[clean]) for f in FIELDS):
      first = t
  print('measured: %s fp%d%s fused against sequential over %d steps x %d envs: first step that differs %s; compared to the '
        'end %d environments, their solves %d, Newton iterations %d, solves past the row cap %d'
        % (name, precision, '' if cap is None else ' ls_iterations=%d' % cap, T, B, first, int(clean.sum()), solves, iters, over))
  assert first is None, '%s: first difference at step %d' % (name, first)
  assert solves > 0 and iters > 0
  assert np.isfinite(fused.get('qpos')).all()
  return over


@pytest.mark.parametrize('name', nr.BAKED)
def test_fp32_fused_search_is_bit_identical_to_the_sequential_search(monkeypatch, name):
  m = nr._model(name)
  fused = nr._default(monkeypatch, m, name, B, 32)
  seq = nr._plugin(monkeypatch, m, B, 32, SEQ_FLAGS)
  assert seq.info()['lanes_per_env'] == fused.info()['lanes_per_env']
  _compare(monkeypatch, name, 32, fused, seq)
  fused.close(); seq.close()


@pytest.mark.parametrize('name', nr.BAKED)
def test_fp64_fused_search_is_bit_identical_to_the_sequential_search(monkeypatch, name):
  m = nr._model(name)
  fused = nr._plugin(monkeypatch, m, B, 64, nr.F64_REGS_FLAGS)
  seq = nr._plugin(monkeypatch, m, B, 64, nr.F64_REGS_FLAGS + ' ' + SEQ_FLAGS)
  assert seq.info()['lanes_per_env'] == fused.info()['lanes_per_env']
  _compare(monkeypatch, name, 64, fused, seq)
  fused.close(); seq.close()


def test_fp32_under_a_cap_of_four_evaluations(monkeypatch):
  m = nr._model('cheetah')
  fused = nr._default(monkeypatch, m, 'cheetah', B, 32)
  seq = nr._plugin(monkeypatch, m, B, 32, SEQ_FLAGS)
  _compare(monkeypatch, 'cheetah', 32, fused, seq, cap=4)
  fused.close(); seq.close()


def test_fp32_chain_that_leaves_the_register_rows_inside_a_wave(monkeypatch):
  m = nr._model('chain')
  fused = nr._default(monkeypatch, m, 'chain', B, 32)
  seq = nr._plugin(monkeypatch, m, B, 32, SEQ_FLAGS)
  assert seq.info()['lanes_per_env'] == fused.info()['lanes_per_env']
  over = _compare(monkeypatch, 'chain', 32, fused, seq, rows_cap=16)
  assert over > 0      # the LDS fallback ran next to the register rows
  fused.close(); seq.close()

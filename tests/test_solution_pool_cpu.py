"""The solution pool (miqp_solver_set_pool, _pool_count, _pool_found, _pool_solve, _pool_record), as far as it can be checked without a device: its
exports, the capacity setting and every answer that is decided before a device is asked for.  What it keeps and computes: test_solution_pool_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import FixedResultC, RawResults

NAMES = ("miqp_solver_set_pool", "miqp_solver_pool_count", "miqp_solver_pool_found", "miqp_solver_pool_solve", "miqp_solver_pool_record", "miqp_gpu_pool_max")


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def _loaded():
    w = P.CplexWrapper(); w.resetParameters(synthetic.generate("mini", 0))
    assert w._push_inputs() == 0
    return w


def test_the_exports_exist(lib):
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS


def test_the_maximum_is_a_build_constant_of_at_least_eight(lib):
    assert lib.miqp_gpu_pool_max() >= 8
    assert P.pool_max() == lib.miqp_gpu_pool_max()


def test_set_pool_refuses_what_is_out_of_range_and_keeps_the_setting(lib):
    w = _loaded()
    top = lib.miqp_gpu_pool_max()
    assert lib.miqp_solver_set_pool(None, 4) < 0
    assert lib.miqp_solver_set_pool(w._h, 5) == 0
    assert lib.miqp_solver_set_pool(w._h, -1) < 0
    assert lib.miqp_solver_set_pool(w._h, top + 1) < 0
    # (the setting is not readable by itself: that a refused call leaves the accepted one before it in force shows in the count of the next solve -
    # test_solution_pool_gpu.py::test_a_refused_capacity_leaves_the_previous_one_in_force)
    assert w.setSolutionPool(top + 1) < 0 and w.setSolutionPool(top) == 0 and w.setSolutionPool(0) == 0
    # ... and the C++ adapter's rule is the library's: the two ends of the range are accepted
    assert lib.miqp_solver_set_pool(w._h, top) == 0 and lib.miqp_solver_set_pool(w._h, 0) == 0


def test_the_count_is_zero_without_a_solve(lib):
    empty = P.CplexWrapper()
    assert lib.miqp_solver_pool_count(empty._h) == 0 and lib.miqp_solver_pool_count(None) == 0
    w = _loaded()
    assert w.solutionPoolCount() == 0            # pool off, no solve
    assert w.setSolutionPool(8) == 0
    assert w.solutionPoolCount() == 0            # pool on, no solve
    assert w._push_inputs() == 0                 # new parameters
    assert w.solutionPoolCount() == 0
    assert w.setSolutionPool(0) == 0
    assert w.solutionPoolCount() == 0
    assert len(w.solutionPoolFound()) == 0
    o = (C.c_double * 4)()
    assert lib.miqp_solver_pool_found(w._h, o, 4) == 0
    assert lib.miqp_solver_pool_found(w._h, None, 4) == -1 and lib.miqp_solver_pool_found(None, o, 4) == -1


def test_record_and_solve_give_their_error_codes_on_a_handle_without_a_pool(lib):
    w = _loaded()
    r = RawResults(2, 8, 32, 1, 0, 0)
    assert lib.miqp_solver_pool_record(w._h, 0, C.byref(r.to_c())) == -1
    assert lib.miqp_solver_pool_record(None, 0, C.byref(r.to_c())) == -1
    assert lib.miqp_solver_pool_record(w._h, 0, None) == -1
    assert w.solutionPoolRecord(0) == (-1, None)
    out = (FixedResultC * 2)()
    assert lib.miqp_solver_pool_solve(None, out, 2) == -1
    assert lib.miqp_solver_pool_solve(w._h, None, 2) == -1
    assert lib.miqp_solver_pool_solve(w._h, out, 0) == -1
    assert lib.miqp_solver_pool_solve(P.CplexWrapper()._h, out, 2) == -1     # a handle without an instance


def test_no_device_no_answer(lib):
    """without a HIP device a well-formed call fails loudly with -3: there is no host solve"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    w = _loaded()
    w.setSolutionPool(4)
    out = (FixedResultC * 4)()
    assert lib.miqp_solver_pool_solve(w._h, out, 4) == -3
    with pytest.raises(RuntimeError):
        w.solveSolutionPool()
    assert w.solutionPoolRecord(0) == (-1, None)


def test_the_wrapper_methods_forward(lib):
    w = _loaded()
    for n in ("setSolutionPool", "solutionPoolCount", "solveSolutionPool", "solutionPoolRecord", "solutionPoolFound"):
        assert callable(getattr(w, n)), n
    assert w.setSolutionPool(3) == lib.miqp_solver_set_pool(w._h, 3) == 0
    assert w.setSolutionPool(-2) == lib.miqp_solver_set_pool(w._h, -2) < 0
    assert w.solutionPoolCount() == lib.miqp_solver_pool_count(w._h) == 0
    assert isinstance(w.solutionPoolFound(), np.ndarray)

"""The batch form of solveFixed (miqp_solver_solve_fixed_batch), as far as it can be checked without a device: its exports, the struct of its
answers, the size of its launch groups, and every refusal that is decided before a device is asked for.  What it computes: test_fixed_batch_gpu.py."""
import ctypes as C
import math

import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import FixedResultC, RawResults, RawResultsC

CAP = 65536   # entries per call (include/miqp_gpu.h)


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def _loaded():
    w = P.CplexWrapper(); w.resetParameters(synthetic.generate("mini", 0))
    assert w._push_inputs() == 0
    return w


def _records(n, dims=(2, 8, 32, 1, 0, 0)):
    recs = [RawResults(*dims) for _ in range(n)]
    keep = [r.to_c() for r in recs]
    return recs, keep, (C.POINTER(RawResultsC) * n)(*[C.pointer(c) for c in keep])


def test_the_four_exports_exist(lib):
    for n in ("miqp_solver_solve_fixed_batch", "miqp_solver_fixed_batch_record", "miqp_gpu_fixed_result_size", "miqp_gpu_fixed_batch_chunk"):
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS


def test_the_struct_has_the_size_the_library_says(lib):
    assert lib.miqp_gpu_fixed_result_size() == C.sizeof(FixedResultC) == 32


def test_the_chunk_is_within_its_limits(lib):
    assert 64 <= P.fixed_batch_chunk() <= CAP
    assert P.fixed_batch_chunk() == lib.miqp_gpu_fixed_batch_chunk()


def test_refusals_need_no_device(lib):
    recs, keep, ptrs = _records(2)
    out = (FixedResultC * 2)()
    best = C.c_int(7)
    empty = P.CplexWrapper()                       # a handle without an instance
    assert lib.miqp_solver_solve_fixed_batch(empty._h, ptrs, 2, out, C.byref(best)) == -1
    assert lib.miqp_solver_solve_fixed_batch(None, ptrs, 2, out, C.byref(best)) == -1
    w = _loaded()
    assert lib.miqp_solver_solve_fixed_batch(w._h, ptrs, 0, out, C.byref(best)) == -1
    assert lib.miqp_solver_solve_fixed_batch(w._h, ptrs, -3, out, C.byref(best)) == -1
    assert lib.miqp_solver_solve_fixed_batch(w._h, None, 2, out, C.byref(best)) == -1
    assert lib.miqp_solver_solve_fixed_batch(w._h, ptrs, 2, None, C.byref(best)) == -1
    # above the cap: refused before either array is read (they hold two entries)
    assert lib.miqp_solver_solve_fixed_batch(w._h, ptrs, CAP + 1, out, C.byref(best)) == -5
    # no batch call yet: no record to hand out
    r = RawResults(2, 8, 32, 1, 0, 0)
    assert lib.miqp_solver_fixed_batch_record(w._h, 0, C.byref(r.to_c())) == -1
    assert lib.miqp_solver_fixed_batch_record(None, 0, C.byref(r.to_c())) == -1
    assert w.fixedBatchRecord(0) == (-1, None)


def test_a_call_of_refused_entries_alone_succeeds_without_a_device(lib):
    """a refused ENTRY does not fail the call: records of another shape and a NULL record are status 2, nothing is left to run, best is -1"""
    w = _loaded()
    recs, keep, ptrs = _records(2, dims=(2, 9, 32, 1, 0, 0))      # another horizon
    three = (C.POINTER(RawResultsC) * 3)(ptrs[0], None, ptrs[1])
    out = (FixedResultC * 3)()
    best = C.c_int(7)
    assert lib.miqp_solver_solve_fixed_batch(w._h, three, 3, out, C.byref(best)) == 0
    assert [o.status for o in out] == [2, 2, 2] and [o.route for o in out] == [-1, -1, -1] and best.value == -1
    assert all(math.isnan(o.objective) and math.isnan(o.violation) for o in out)
    r = RawResults(2, 8, 32, 1, 0, 0)
    assert lib.miqp_solver_fixed_batch_record(w._h, 0, C.byref(r.to_c())) == -1   # (no entry ran: nothing is held)


def test_no_device_no_answer(lib):
    """without a HIP device a well-formed call fails loudly with -3 and every entry reads "not run" (status 2, never 0 = feasible): there is no
    host solve"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    w = _loaded()
    recs, keep, ptrs = _records(3)
    out = (FixedResultC * 3)()
    for o in out:
        o.status = 0
    best = C.c_int(0)
    assert lib.miqp_solver_solve_fixed_batch(w._h, ptrs, 3, out, C.byref(best)) == -3
    assert [o.status for o in out] == [2, 2, 2] and best.value == -1
    with pytest.raises(RuntimeError):
        w.solveFixedBatch(recs)
    assert w.fixedBatchRecord(0) == (-1, None)

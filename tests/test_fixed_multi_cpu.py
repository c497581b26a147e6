"""The fix records and solution pools of many handles in one call (miqp_solver_solve_fixed_multi, miqp_solver_pool_solve_multi), as far as they can
be checked without a device: the exports and their bindings, every refusal that is decided before a device is asked for - and that a refused call
leaves what the handles keep alone - and the calls with nothing to run.  What they compute: test_fixed_multi_gpu.py."""
import ctypes as C
import math
import os
import re

import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import FixedResultC, RawResults, RawResultsC

CAP = 65536   # entries per call (include/miqp_gpu.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = (2, 8, 32, 1, 0, 0)


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def _loaded(cfg="mini", seed=0, **kw):
    w = P.CplexWrapper(**kw); w.resetParameters(synthetic.generate(cfg, seed))
    assert w._push_inputs() == 0
    return w


def _records(n, dims=MINI):
    recs = [RawResults(*dims) for _ in range(n)]
    keep = [r.to_c() for r in recs]
    return recs, keep, (C.POINTER(RawResultsC) * max(n, 1))(*[C.pointer(c) for c in keep])


def _handles(ws):
    return (C.c_void_p * len(ws))(*[w._h for w in ws])


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _kept(w):
    """what a handle keeps for its record calls and its pool, as far as it can be read"""
    return (w.fixedBatchRecord(0)[0], w.solutionPoolRecord(0)[0], w.solutionPoolCount(), w.lastError())


def test_the_exports_exist_and_bind(lib):
    hdr = open(os.path.join(ROOT, "include", "miqp_gpu.h")).read()
    for n in ("miqp_solver_solve_fixed_multi", "miqp_solver_pool_solve_multi"):
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS
        assert getattr(lib, n).restype is C.c_int and getattr(lib, n).argtypes
        assert re.search(r"\bint\s+%s\s*\(\s*miqp_solver_t\s*\*\s*const\s*\*\s*solvers\s*,\s*int\s+n\s*," % n, hdr), n
    assert len(lib.miqp_solver_solve_fixed_multi.argtypes) == 6 and len(lib.miqp_solver_pool_solve_multi.argtypes) == 5
    assert callable(P.solve_fixed_multi) and callable(P.solve_solution_pools)


def test_fixed_multi_refuses_before_a_device_is_asked_for(lib):
    f = lib.miqp_solver_solve_fixed_multi
    a, b = _loaded(seed=0), _loaded(seed=1)
    recs, keep, ptrs = _records(4)
    out = (FixedResultC * 4)()
    for o in out:
        o.status = 9
    best = _ints(7, 7)
    hs, first = _handles([a, b]), _ints(0, 2, 4)
    before = [_kept(w) for w in (a, b)]
    # -1: NULL arguments, n <= 0
    assert f(None, 2, ptrs, first, out, best) == -1
    assert f(hs, 2, None, first, out, best) == -1
    assert f(hs, 2, ptrs, None, out, best) == -1
    assert f(hs, 2, ptrs, first, None, best) == -1
    assert f(hs, 0, ptrs, first, out, best) == -1
    assert f(hs, -2, ptrs, first, out, best) == -1
    # -1: a NULL handle, a handle without an instance, a handle named twice
    assert f((C.c_void_p * 2)(a._h, None), 2, ptrs, first, out, best) == -1
    assert f(_handles([a, P.CplexWrapper()]), 2, ptrs, first, out, best) == -1
    assert f(_handles([a, a]), 2, ptrs, first, out, best) == -1
    # -1: a `first` that does not start at 0, or descends
    assert f(hs, 2, ptrs, _ints(1, 2, 4), out, best) == -1
    assert f(hs, 2, ptrs, _ints(0, 3, 2), out, best) == -1
    # -2: another shape (one car), with batch_layout's text; another device
    c = _loaded("mini1", 0)
    assert f(_handles([a, c]), 2, ptrs, first, out, best) == -2
    assert "share" in a.lastError() and a.lastError() == c.lastError()
    before[0] = _kept(a)   # (the refusal's text is the handle's last error from here on)
    d0, d1 = _loaded(seed=2, device=0), _loaded(seed=3, device=1)
    assert f(_handles([d0, d1]), 2, ptrs, first, out, best) == -2
    assert "device" in d0.lastError()
    # -5: more entries than a call takes, refused before either array is read (they hold four entries)
    assert f(hs, 2, ptrs, _ints(0, 2, CAP + 1), out, best) == -5
    # nothing was written, nothing the handles keep has changed
    assert [o.status for o in out] == [9] * 4 and list(best) == [7, 7]
    assert [_kept(w) for w in (a, b)] == before


def test_pool_multi_refuses_before_a_device_is_asked_for(lib):
    f = lib.miqp_solver_pool_solve_multi
    a, b = _loaded(seed=0), _loaded(seed=1)
    out = (FixedResultC * 8)()
    for o in out:
        o.status = 9
    counts = _ints(7, 7)
    hs = _handles([a, b])
    before = [_kept(w) for w in (a, b)]
    assert f(None, 2, out, 4, counts) == -1
    assert f(hs, 2, None, 4, counts) == -1
    assert f(hs, 2, out, 4, None) == -1
    assert f(hs, 0, out, 4, counts) == -1
    assert f(hs, 2, out, 0, counts) == -1
    assert f((C.c_void_p * 2)(a._h, None), 2, out, 4, counts) == -1
    assert f(_handles([a, P.CplexWrapper()]), 2, out, 4, counts) == -1
    assert f(_handles([a, a]), 2, out, 4, counts) == -1
    c = _loaded("mini1", 0)
    assert f(_handles([a, c]), 2, out, 4, counts) == -2
    before[0] = _kept(a)
    d0, d1 = _loaded(seed=2, device=0), _loaded(seed=3, device=1)
    assert f(_handles([d0, d1]), 2, out, 4, counts) == -2
    assert [o.status for o in out] == [9] * 8 and list(counts) == [7, 7]
    assert [_kept(w) for w in (a, b)] == before


def test_calls_with_nothing_to_run_return_0_without_a_device(lib):
    """every range empty; every entry refused (a NULL record, records of another horizon): 0, best -1 for every handle, refused entries status 2;
    handles without a pool: 0 and counts 0.  None of it needs or touches a device"""
    a, b, c = _loaded(seed=0), _loaded(seed=1), _loaded(seed=2)
    hs = _handles([a, b, c])
    recs, keep, ptrs = _records(2, dims=(2, 9, 32, 1, 0, 0))
    out = (FixedResultC * 3)()
    for o in out:
        o.status = 9
    best = _ints(7, 7, 7)
    assert lib.miqp_solver_solve_fixed_multi(hs, 3, ptrs, _ints(0, 0, 0, 0), out, best) == 0
    assert list(best) == [-1, -1, -1] and [o.status for o in out] == [9] * 3
    three = (C.POINTER(RawResultsC) * 3)(ptrs[0], None, ptrs[1])
    best = _ints(7, 7, 7)
    assert lib.miqp_solver_solve_fixed_multi(hs, 3, three, _ints(0, 2, 2, 3), out, best) == 0
    assert list(best) == [-1, -1, -1]
    assert [o.status for o in out] == [2, 2, 2] and [o.route for o in out] == [-1, -1, -1]
    assert all(math.isnan(o.objective) and math.isnan(o.violation) for o in out)
    assert all(w.fixedBatchRecord(0) == (-1, None) for w in (a, b, c))   # (no entry ran: nothing is held)
    counts = _ints(7, 7, 7)
    pout = (FixedResultC * 12)()
    for o in pout:
        o.status = 9
    assert lib.miqp_solver_pool_solve_multi(hs, 3, pout, 4, counts) == 0
    assert list(counts) == [0, 0, 0] and [o.status for o in pout] == [9] * 12
    # ... and through the module functions
    res = P.solve_fixed_multi([a, b, c], [[], [None], []])
    assert [len(r[0]) for r in res] == [0, 1, 0] and [r[5] for r in res] == [-1, -1, -1] and res[1][0][0] == 2
    assert [len(r[0]) for r in P.solve_solution_pools([a, b, c])] == [0, 0, 0]


def test_no_device_no_answer(lib):
    """a well-formed call with something to run: on a machine without a HIP device it fails loudly with -3 and every entry reads "not run" (status 2,
    never 0 = feasible), there is no host solve; with a device it runs (what it answers: test_fixed_multi_gpu.py)"""
    import torch
    a, b = _loaded(seed=0), _loaded(seed=1)
    recs, keep, ptrs = _records(3)
    out = (FixedResultC * 3)()
    for o in out:
        o.status = 0
    best = _ints(0, 0)
    rc = lib.miqp_solver_solve_fixed_multi(_handles([a, b]), 2, ptrs, _ints(0, 1, 3), out, best)
    if torch.cuda.is_available():
        assert rc == 0 and all(o.status in (0, 1) for o in out)
        return
    assert rc == -3
    assert [o.status for o in out] == [2, 2, 2] and list(best) == [-1, -1]
    with pytest.raises(RuntimeError):
        P.solve_fixed_multi([a, b], [recs[:1], recs[1:]])
    assert a.fixedBatchRecord(0) == (-1, None) and b.fixedBatchRecord(0) == (-1, None)

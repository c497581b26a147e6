"""Settled labels (miqp_solver_settle_decisions) and the explore with settled admission (miqp_solver_pool_explore_settled), as far as they can be
checked without a device: the exports, header and bindings, the number of settle passes, and every answer of both calls that is
decided before a device is asked for.  What the device does: test_pool_settle_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd.ctypes_types import PoolExploreC
from test_pool_label_cpu import BP, _loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("miqp_solver_settle_decisions", "miqp_solver_pool_explore_settled", "miqp_gpu_pool_settle_passes")
IP = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def test_the_exports_exist(lib):
    hdr = open(os.path.join(ROOT, "include", "miqp_gpu.h")).read()
    hpp = open(os.path.join(ROOT, "include", "cplex_wrapper.hpp")).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS
        assert n + "(" in hdr, n
    assert "settleDecisions" in hpp and "exploreSolutionPoolSettled" in hpp
    assert callable(P.CplexWrapper.settleDecisions) and callable(P.pool_settle_passes)
    assert os.path.exists(os.path.join(ROOT, "planner_miqp_amd", "csrc", "pool_settle.hip"))
    for text in ("miqp_solver_fixed_batch_record", "out[k] is the LAST solve", "out[k].reserved"):   # what the header promises about state and records
        assert text in hdr, text


def test_the_settle_passes_are_the_refinements(lib):
    assert lib.miqp_gpu_pool_settle_passes() == 6 == P.pool_settle_passes()
    src = open(os.path.join(ROOT, "planner_miqp_amd", "csrc", "solution_pool.hip")).read()
    assert "constexpr int POOL_PASSES = 6;" in src   # one constant: the refinement's


def test_settle_decisions_without_a_device(lib):
    import torch
    w, dims = _loaded()
    D = P.wrapper._decision_len(dims[0], dims[1], dims[4])
    rec = np.full((3, D), -1, dtype=np.int8)
    out = (P.FixedResultC * 3)()
    settled = np.zeros((3, D), dtype=np.int8); solves = np.full(3, 9, dtype=np.int32)
    f = lib.miqp_solver_settle_decisions
    rp, sp, np_ = rec.ctypes.data_as(BP), settled.ctypes.data_as(BP), solves.ctypes.data_as(IP)
    assert f(None, rp, 3, out, sp, np_, None) == -1 and f(w._h, None, 3, out, sp, np_, None) == -1 and f(w._h, rp, 3, None, sp, np_, None) == -1
    assert f(w._h, rp, 3, out, None, np_, None) == -1 and f(w._h, rp, 3, out, sp, None, None) == -1
    assert f(w._h, rp, 0, out, sp, np_, None) == -1 and f(w._h, rp, -1, out, sp, np_, None) == -1
    assert f(w._h, rp, 65537, out, sp, np_, None) == -5
    assert f(P.CplexWrapper()._h, rp, 3, out, sp, np_, None) == -1   # no instance
    assert list(solves) == [9, 9, 9]   # (a refused call writes nothing)
    bad = rec.copy(); bad[:, 1] = 127   # no car has that many possible regions: refused on the host, no device is asked for
    rc, status, obj, viol, it, route, best, settled, solves = w.settleDecisions(bad)
    assert rc == 0 and list(status) == [2, 2, 2] and best == -1 and np.isnan(obj).all() and list(route) == [-1, -1, -1]
    assert settled.shape == (3, D) and settled.dtype == np.int8 and (settled == -1).all()
    assert solves.shape == (3,) and solves.dtype == np.int32 and (solves == 0).all()
    with pytest.raises(ValueError):
        w.settleDecisions(rec[:, :-1])
    if not torch.cuda.is_available():
        rc, status, obj, viol, it, route, best, settled, solves = w.settleDecisions(rec)
        assert rc == -3 and list(status) == [2, 2, 2] and best == -1 and np.isnan(obj).all() and (settled == -1).all() and (solves == 0).all()
    # the answers decided on the host are those of canonicalDecisions
    a, b = w.canonicalDecisions(bad), w.settleDecisions(bad)
    assert a[0] == b[0] and a[6] == b[6] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:6], b[1:6])) and a[7].tobytes() == b[7].tobytes()


def test_settled_explore_answers_before_any_device(lib):
    """every -1 / -2 / 0 answer of the plain call (test_pool_explore_cpu.py), through the settled entry; distinct and settled together are refused"""
    w, _ = _loaded()
    assert w.setSolutionPool(8) == 0
    out = (PoolExploreC * 16)()
    f = lib.miqp_solver_pool_explore_settled
    assert f(None, 4, -1.0, out, 16) == -1 and f(w._h, 4, -1.0, None, 16) == -1
    assert f(w._h, 4, -1.0, out, -1) == -1 and f(w._h, 4, float("nan"), out, 16) == -1
    for fam in (0, 1, 2, 3, 16, 28, 31):
        assert w.setSolutionPoolFilter(fam) == 0
        rc, added = w.exploreSolutionPool(settled=True)
        assert rc == -2 and added == [], (fam, rc)
        assert w.solutionPoolCount() == 0 and len(w.solutionPoolFound()) == 0
    for fam in (4, 8, 12, 15):
        assert w.setSolutionPoolFilter(fam) == 0
        for passes in (0, -1, 65):
            assert w.exploreSolutionPool(passes, settled=True)[0] == -2, (fam, passes)
        assert w.exploreSolutionPool(settled=True) == (0, []) and w.exploreSolutionPool(1, 0.5, False, True) == (0, [])   # (no solve yet: the pool is empty, with or without a device)
        assert w.solutionPoolCount() == 0 and w.solutionPoolFoundDecisions(0) is None
        with pytest.raises(ValueError):
            w.exploreSolutionPool(distinct=True, settled=True)
    import torch
    if not torch.cuda.is_available():
        assert w.callCplex() != P.OptimizationStatus.SUCCESS and w.exploreSolutionPool(settled=True) == (0, []) and w.solutionPoolCount() == 0
    assert f(P.CplexWrapper()._h, 4, -1.0, out, 16) == -1   # no instance
    assert w.exploreSolutionPool() == (0, []) and w.exploreSolutionPool(distinct=True) == (0, [])   # (the other two modes are what they were)

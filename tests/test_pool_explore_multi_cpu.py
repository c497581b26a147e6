"""The free places of the solution pools of many handles filled in one call (miqp_solver_pool_explore_multi, miqp_gpu_pool_explore_plan; DESIGN.md
6k), as far as it can be checked without a device: the exports, their bindings and the three mode constants, the slices of a pass against a numpy
restatement of the greedy rule, every refusal that is decided before a device is asked for and can be provoked without a pool - and that a refused
call leaves its arrays and what the handles keep alone - and the call with nothing to run.  A handle has entries only behind a solve, so the refusals
that need some (the filter without jumps, a cap below the free places) and what the call computes are in test_pool_explore_multi_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import PoolExploreC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB_MAX = 8192      # neighbours of a slice: 16 places of 512 jumps (include/miqp_gpu.h)
HANDLES_MAX = 4096  # 65536 places of 16 per handle


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def _loaded(cfg="mini", seed=0, **kw):
    w = P.CplexWrapper(**kw); w.resetParameters(synthetic.generate(cfg, seed))
    assert w._push_inputs() == 0
    return w


def _handles(ws):
    return (C.c_void_p * len(ws))(*[w._h for w in ws])


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _kept(w):
    """what a handle keeps for its pool, as far as it can be read"""
    return (w.solutionPoolRecord(0)[0], w.solutionPoolCount(), w.lastError())


def _marked(n):
    out = (PoolExploreC * n)()
    for o in out:
        o.parent = 9; o.pass_ = 9
    return out


def _greedy(totals):
    """the rule restated: handles in order; a handle opens a new slice when its neighbours do not fit the 8192 results of the current one"""
    c = np.asarray(totals, dtype=np.int64)
    first, room = [0], NB_MAX
    for h, x in enumerate(c):
        if x > room:
            first.append(h); room = NB_MAX
        room -= int(x)
    return first + [len(c)]


def test_the_exports_exist_and_bind(lib):
    hdr = open(os.path.join(ROOT, "include", "miqp_gpu.h")).read()
    for n in ("miqp_solver_pool_explore_multi", "miqp_gpu_pool_explore_plan"):
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS
        assert getattr(lib, n).restype is C.c_int and getattr(lib, n).argtypes
    assert len(lib.miqp_solver_pool_explore_multi.argtypes) == 8 and len(lib.miqp_gpu_pool_explore_plan.argtypes) == 4
    assert re.search(r"\bint\s+miqp_solver_pool_explore_multi\s*\(\s*miqp_solver_t\s*\*\s*const\s*\*\s*solvers\s*,\s*int\s+n\s*,\s*int\s+mode\s*,\s*int\s+max_passes\s*,"
                     r"\s*double\s+max_rel\s*,\s*miqp_pool_explore_c\s*\*\s*out\s*,\s*int\s+cap\s*,\s*int\s*\*\s*counts\s*\)", hdr)
    assert re.search(r"\bint\s+miqp_gpu_pool_explore_plan\s*\(\s*const\s+int\s*\*\s*handle_totals\s*,\s*int\s+n\s*,\s*int\s*\*\s*slice_first\s*,\s*int\s+cap\s*\)", hdr)
    # the three modes, in the header and in the package, with the values the library's table of admissions is indexed by
    for name, value in (("PLAIN", 0), ("DISTINCT", 1), ("SETTLED", 2)):
        assert re.search(r"#define\s+MIQP_POOL_EXPLORE_%s\s+%d\b" % (name, value), hdr), name
        assert getattr(P, "POOL_EXPLORE_" + name) == value
    assert "checks the filter first" in hdr   # (the one difference to the single call is said where the call is declared)
    assert callable(P.explore_solution_pools) and callable(P.pool_explore_plan)
    assert P.explore_solution_pools is P.wrapper.explore_solution_pools and P.pool_explore_plan is P.wrapper.pool_explore_plan


@pytest.mark.parametrize("length", [1, 2, 17, 1000, 4096])
def test_plan_is_the_greedy_rule_on_random_totals(lib, length):
    rng = np.random.default_rng(2000 + length)
    for trial in range(3):
        c = rng.integers(0, NB_MAX + 1, size=length)
        if trial == 2:   # many handles without neighbours, as a call in its later passes has them
            c[rng.random(length) < 0.7] = 0
        first = P.pool_explore_plan(c)
        assert first == _greedy(c), (length, trial)
        assert first[0] == 0 and first[-1] == length and all(a < b for a, b in zip(first, first[1:]))
        tot = np.concatenate([[0], np.cumsum(c)])
        sizes = [int(tot[b] - tot[a]) for a, b in zip(first, first[1:])]
        assert max(sizes) <= NB_MAX
        # greedy: the first handle of every further slice did not fit the slice before
        assert all(sizes[s] + int(c[first[s + 1]]) > NB_MAX for s in range(len(sizes) - 1))


def test_plan_edges(lib):
    assert P.pool_explore_plan(np.zeros(4096, dtype=np.int32)) == [0, 4096]                  # all zeros: one slice
    assert P.pool_explore_plan([0]) == [0, 1] and P.pool_explore_plan([NB_MAX]) == [0, 1]
    assert P.pool_explore_plan(np.full(100, NB_MAX)) == list(range(101))                     # all 8192: a slice per handle
    assert P.pool_explore_plan([4096, 4095, 1]) == [0, 3]                                    # a total of exactly 8192
    assert P.pool_explore_plan([4096, 4095, 2]) == [0, 2, 3]                                 # ... and of 8193
    assert P.pool_explore_plan([4096, 4095, 1, 0, 0, 1]) == [0, 5, 6]                        # (a handle without neighbours rides along in a full slice)
    assert P.pool_explore_plan([0, 0, NB_MAX, 0, NB_MAX, 0]) == [0, 4, 6]
    assert P.pool_explore_plan([2782, 2186, 2017, 1783, 1283]) == [0, 3, 5]                  # (the five cfg4 seeds of the GPU suite's two slices)


def test_plan_error_codes(lib):
    f = lib.miqp_gpu_pool_explore_plan
    c = _ints(*([NB_MAX] * 3))
    first = _ints(*([77] * 8))
    assert f(None, 3, first, 8) == -1 and f(c, 3, None, 8) == -1
    assert f(c, 0, first, 8) == -1 and f(c, -3, first, 8) == -1 and f(c, 3, first, -1) == -1
    # a total outside 0 .. 8192: -2, wherever it stands, and nothing written
    for bad in (-1, NB_MAX + 1, 100000):
        for at in range(3):
            t = [5, 5, 5]; t[at] = bad
            assert f(_ints(*t), 3, first, 8) == -2, (bad, at)
    # three slices need four entries of slice_first: -3 below that, and nothing written
    for cap in (0, 1, 2, 3):
        assert f(c, 3, first, cap) == -3, cap
    assert list(first) == [77] * 8
    assert f(c, 3, first, 4) == 3 and list(first) == [0, 1, 2, 3, 77, 77, 77, 77]
    with pytest.raises(ValueError):
        P.pool_explore_plan([])
    with pytest.raises(RuntimeError):
        P.pool_explore_plan([NB_MAX + 1])


def test_refuses_before_a_device_is_asked_for(lib):
    f = lib.miqp_solver_pool_explore_multi
    a, b = _loaded(seed=0), _loaded(seed=1)
    out = _marked(32)
    counts = _ints(7, 7)
    hs = _handles([a, b])
    before = [_kept(w) for w in (a, b)]
    # -1: NULL arrays, n <= 0, cap < 0, max_rel a NaN, mode outside 0 .. 2
    assert f(None, 2, 0, 4, -1.0, out, 16, counts) == -1
    assert f(hs, 2, 0, 4, -1.0, None, 16, counts) == -1
    assert f(hs, 2, 0, 4, -1.0, out, 16, None) == -1
    assert f(hs, 0, 0, 4, -1.0, out, 16, counts) == -1 and f(hs, -2, 0, 4, -1.0, out, 16, counts) == -1
    assert f(hs, 2, 0, 4, -1.0, out, -1, counts) == -1
    assert f(hs, 2, 0, 4, float("nan"), out, 16, counts) == -1
    assert f(hs, 2, -1, 4, -1.0, out, 16, counts) == -1 and f(hs, 2, 3, 4, -1.0, out, 16, counts) == -1
    # -2: max_passes outside 1 .. 64
    for mode in (0, 1, 2):
        assert f(hs, 2, mode, 0, -1.0, out, 16, counts) == -2 and f(hs, 2, mode, 65, -1.0, out, 16, counts) == -2
    # -1: a NULL handle, a handle without an instance, a handle named twice
    assert f((C.c_void_p * 2)(a._h, None), 2, 0, 4, -1.0, out, 16, counts) == -1
    assert f(_handles([a, P.CplexWrapper()]), 2, 0, 4, -1.0, out, 16, counts) == -1
    assert f(_handles([a, a]), 2, 0, 4, -1.0, out, 16, counts) == -1
    assert [_kept(w) for w in (a, b)] == before
    # -5: more than 4096 handles (the array is not read that far: it is refused on its length)
    assert f(hs, HANDLES_MAX + 1, 0, 4, -1.0, out, 16, counts) == -5
    # -2: another shape (one car), with batch_layout's text; another device
    c = _loaded("mini1", 0)
    assert f(_handles([a, c]), 2, 0, 4, -1.0, out, 16, counts) == -2
    assert "share" in a.lastError() and a.lastError() == c.lastError()
    before[0] = _kept(a)   # (the refusal's text is the handle's last error from here on)
    d0, d1 = _loaded(seed=2, device=0), _loaded(seed=3, device=1)
    assert f(_handles([d0, d1]), 2, 2, 4, -1.0, out, 16, counts) == -2
    assert "device" in d0.lastError()
    # nothing was written, nothing the handles keep has changed
    assert [(o.parent, o.pass_) for o in out] == [(9, 9)] * 32 and list(counts) == [7, 7]
    assert [_kept(w) for w in (a, b)] == before
    # ... and through the module function: an exception with the library's text on -2
    with pytest.raises(RuntimeError, match="share"):
        P.explore_solution_pools([a, c])
    with pytest.raises(RuntimeError):
        P.explore_solution_pools([a, b], max_passes=0)
    with pytest.raises(RuntimeError):
        P.explore_solution_pools([a, b], max_rel=float("nan"))


def test_distinct_and_settled_together_are_refused(lib):
    a = _loaded(seed=0)
    with pytest.raises(ValueError):
        P.explore_solution_pools([a], distinct=True, settled=True)
    with pytest.raises(ValueError):
        P.explore_solution_pools([], distinct=True, settled=True)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_handles_without_pools_return_0_without_a_device(lib, mode):
    """no handle has entries - pool off, no solve - whatever the filters, filter 0 and the timing bit included: no handle takes part, so the call
    returns 0, every count 0, nothing written to `out`, a last error cleared as the single call clears it; none of it needs a device"""
    a, b, c, d = _loaded(seed=0), _loaded(seed=1), _loaded(seed=2), _loaded(seed=3)
    assert b.setSolutionPoolFilter(12) == 0 and c.setSolutionPool(4) == 0 and d.setSolutionPoolFilter(16 + 12) == 0
    # a last error from an earlier refusal: the call speaks for every handle from here on
    assert lib.miqp_solver_pool_explore_multi(_handles([a, _loaded("mini1", 0)]), 2, mode, 4, -1.0, _marked(32), 16, _ints(7, 7)) == -2
    assert a.lastError()
    before = [_kept(w)[:2] for w in (a, b, c, d)]
    out = _marked(64)
    counts = _ints(7, 7, 7, 7)
    assert lib.miqp_solver_pool_explore_multi(_handles([a, b, c, d]), 4, mode, 4, 0.5, out, 16, counts) == 0
    assert list(counts) == [0, 0, 0, 0] and [(o.parent, o.pass_) for o in out] == [(9, 9)] * 64
    assert [_kept(w)[:2] for w in (a, b, c, d)] == before
    assert [w.lastError() for w in (a, b, c, d)] == [""] * 4
    # cap 0 is enough when nothing takes part
    assert lib.miqp_solver_pool_explore_multi(_handles([a, b]), 2, mode, 1, -1.0, out, 0, counts) == 0
    res = P.explore_solution_pools([a, b, c, d], distinct=mode == 1, settled=mode == 2)
    assert res == [(0, [])] * 4

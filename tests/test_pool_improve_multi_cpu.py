"""The climb of the solution pools of many handles in one call (miqp_solver_pool_improve_multi, miqp_gpu_pool_improve_plan), as far as it
can be checked without a device: the exports and their bindings, the slices of a pass against a numpy restatement of the greedy rule, every refusal
that is decided before a device is asked for - and that a refused call leaves its arrays and what the handles keep alone - and the call with nothing
to run.  What the call computes: test_pool_improve_multi_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import PoolImproveC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB_MAX = 8192      # results of a slice: 16 entries of 512 moves (include/miqp_gpu.h)
MOVES_MAX = 512


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
    """what a handle keeps for its record calls and its pool, as far as it can be read"""
    return (w.fixedBatchRecord(0)[0], w.solutionPoolRecord(0)[0], w.solutionPoolCount(), w.lastError())


def _greedy(counts):
    """the rule restated: entries in order; an entry opens a new slice when its clamped moves do not fit the 8192 results of the current one"""
    c = np.clip(np.asarray(counts, dtype=np.int64), 0, MOVES_MAX)
    first, room = [0], NB_MAX
    for e, x in enumerate(c):
        if x > room:
            first.append(e); room = NB_MAX
        room -= int(x)
    return first + [len(c)]


def test_the_exports_exist_and_bind(lib):
    hdr = open(os.path.join(ROOT, "include", "miqp_gpu.h")).read()
    for n in ("miqp_solver_pool_improve_multi", "miqp_gpu_pool_improve_plan"):
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS
        assert getattr(lib, n).restype is C.c_int and getattr(lib, n).argtypes
    assert len(lib.miqp_solver_pool_improve_multi.argtypes) == 6 and len(lib.miqp_gpu_pool_improve_plan.argtypes) == 4
    assert re.search(r"\bint\s+miqp_solver_pool_improve_multi\s*\(\s*miqp_solver_t\s*\*\s*const\s*\*\s*solvers\s*,\s*int\s+n\s*,\s*int\s+max_passes\s*,"
                     r"\s*miqp_pool_improve_c\s*\*\s*out\s*,\s*int\s+cap\s*,\s*int\s*\*\s*counts\s*\)", hdr)
    assert re.search(r"\bint\s+miqp_gpu_pool_improve_plan\s*\(\s*const\s+int\s*\*\s*move_counts\s*,\s*int\s+entries\s*,\s*int\s*\*\s*slice_first\s*,\s*int\s+cap\s*\)", hdr)
    assert "WHATEVER ITS FILTER" in hdr   # (the difference from the single call is said where the call is declared)
    assert callable(P.improve_solution_pools) and callable(P.pool_improve_plan)
    assert P.improve_solution_pools is P.wrapper.improve_solution_pools and P.pool_improve_plan is P.wrapper.pool_improve_plan


@pytest.mark.parametrize("length", [1, 16, 17, 1000, 65536])
def test_plan_is_the_greedy_rule_on_random_counts(lib, length):
    rng = np.random.default_rng(1000 + length)
    for trial in range(3):
        c = rng.integers(0, MOVES_MAX + 1, size=length)
        first = P.pool_improve_plan(c)
        assert first == _greedy(c), (length, trial)
        assert first[0] == 0 and first[-1] == length and all(a < b for a, b in zip(first, first[1:]))
        tot = np.concatenate([[0], np.cumsum(c)])
        sizes = [int(tot[b] - tot[a]) for a, b in zip(first, first[1:])]
        assert max(sizes) <= NB_MAX
        # greedy: the first entry of every further slice did not fit the slice before
        assert all(sizes[s] + int(c[first[s + 1]]) > NB_MAX for s in range(len(sizes) - 1))
        assert all(b - a >= 16 for a, b in zip(first[:-1], first[1:-1]))   # (every slice but the last holds at least 16 entries)


def test_plan_edges(lib):
    assert P.pool_improve_plan(np.zeros(70000, dtype=np.int32)) == [0, 70000]             # all zeros: one slice
    assert P.pool_improve_plan([0]) == [0, 1] and P.pool_improve_plan([512]) == [0, 1]
    assert P.pool_improve_plan(np.full(100, 512)) == list(range(0, 100, 16)) + [100]      # all 512: slices of exactly 16 entries
    assert P.pool_improve_plan(np.full(32, 512)) == [0, 16, 32]
    assert P.pool_improve_plan([512] * 15 + [511, 1]) == [0, 17]                          # a total of exactly 8192
    assert P.pool_improve_plan([512] * 15 + [511, 2]) == [0, 16, 17]                      # ... and of 8193
    assert P.pool_improve_plan([512] * 15 + [511, 1, 0, 0, 1]) == [0, 19, 20]             # (zeros still fit a full slice)
    # counts outside 0 .. 512 are clamped as the kernels clamp them
    wild = np.array([-5, 100000, 513, -1, 512] * 20, dtype=np.int32)
    assert P.pool_improve_plan(wild) == _greedy(wild) == _greedy(np.clip(wild, 0, MOVES_MAX))
    assert P.pool_improve_plan([100000] * 17) == [0, 16, 17] and P.pool_improve_plan([-7] * 40000) == [0, 40000]


def test_plan_error_codes(lib):
    f = lib.miqp_gpu_pool_improve_plan
    c = _ints(*([512] * 33))
    first = _ints(*([77] * 8))
    assert f(None, 33, first, 8) == -1 and f(c, 33, None, 8) == -1
    assert f(c, 0, first, 8) == -1 and f(c, -3, first, 8) == -1 and f(c, 33, first, -1) == -1
    # three slices need four entries of slice_first: -3 below that, and nothing written
    for cap in (0, 1, 2, 3):
        assert f(c, 33, first, cap) == -3, cap
    assert list(first) == [77] * 8
    assert f(c, 33, first, 4) == 3 and list(first) == [0, 16, 32, 33, 77, 77, 77, 77]
    with pytest.raises(ValueError):
        P.pool_improve_plan([])


def test_refuses_before_a_device_is_asked_for(lib):
    f = lib.miqp_solver_pool_improve_multi
    a, b = _loaded(seed=0), _loaded(seed=1)
    out = (PoolImproveC * 8)()
    for o in out:
        o.status = 9; o.moves = 9
    counts = _ints(7, 7)
    hs = _handles([a, b])
    before = [_kept(w) for w in (a, b)]
    # -1: NULL arguments, n <= 0, cap < 1
    assert f(None, 2, 8, out, 4, counts) == -1
    assert f(hs, 2, 8, None, 4, counts) == -1
    assert f(hs, 2, 8, out, 4, None) == -1
    assert f(hs, 0, 8, out, 4, counts) == -1 and f(hs, -2, 8, out, 4, counts) == -1
    assert f(hs, 2, 8, out, 0, counts) == -1 and f(hs, 2, 8, out, -1, counts) == -1
    # -2: max_passes outside 1 .. 64
    assert f(hs, 2, 0, out, 4, counts) == -2 and f(hs, 2, 65, out, 4, counts) == -2
    # -1: a NULL handle, a handle without an instance, a handle named twice
    assert f((C.c_void_p * 2)(a._h, None), 2, 8, out, 4, counts) == -1
    assert f(_handles([a, P.CplexWrapper()]), 2, 8, out, 4, counts) == -1
    assert f(_handles([a, a]), 2, 8, out, 4, counts) == -1
    assert [_kept(w) for w in (a, b)] == before
    # -2: another shape (one car), with batch_layout's text; another device
    c = _loaded("mini1", 0)
    assert f(_handles([a, c]), 2, 8, out, 4, counts) == -2
    assert "share" in a.lastError() and a.lastError() == c.lastError()
    before[0] = _kept(a)   # (the refusal's text is the handle's last error from here on)
    d0, d1 = _loaded(seed=2, device=0), _loaded(seed=3, device=1)
    assert f(_handles([d0, d1]), 2, 8, out, 4, counts) == -2
    assert "device" in d0.lastError()
    # nothing was written, nothing the handles keep has changed
    assert [(o.status, o.moves) for o in out] == [(9, 9)] * 8 and list(counts) == [7, 7]
    assert [_kept(w) for w in (a, b)] == before
    # ... and through the module function: an exception with the library's text on -2
    with pytest.raises(RuntimeError, match="share"):
        P.improve_solution_pools([a, c])
    with pytest.raises(RuntimeError):
        P.improve_solution_pools([a, b], max_passes=0)


def test_handles_without_pools_return_0_without_a_device(lib):
    """no handle kept anything - pool off, no solve - whatever the filters: 0, every count 0, nothing written to `out`; none of it needs a device"""
    a, b, c = _loaded(seed=0), _loaded(seed=1), _loaded(seed=2)
    assert b.setSolutionPoolFilter(12) == 0 and c.setSolutionPool(4) == 0
    before = [_kept(w) for w in (a, b, c)]
    out = (PoolImproveC * 12)()
    for o in out:
        o.status = 9
    counts = _ints(7, 7, 7)
    assert lib.miqp_solver_pool_improve_multi(_handles([a, b, c]), 3, 8, out, 4, counts) == 0
    assert list(counts) == [0, 0, 0] and [o.status for o in out] == [9] * 12
    assert [_kept(w) for w in (a, b, c)] == before
    res = P.improve_solution_pools([a, b, c])
    assert [r[0] for r in res] == [0, 0, 0]
    for r in res:
        assert all(len(x) == 0 for x in r[1:]) and r[1].dtype == np.float64 and r[3].dtype == np.int32
    assert P.improve_solution_pools([a], max_passes=1, cap=3)[0][0] == 0

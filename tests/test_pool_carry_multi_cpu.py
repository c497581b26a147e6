"""The pools of many (source, destination) pairs carried in one call (miqp_solver_pool_carry_multi), as far as it can be checked without
a device: the exports, the header's text and the bindings; every refusal that is decided before a device is asked for and can be provoked without a
pool - and that a refused call leaves its arrays and what the handles keep alone -; and the call with nothing to run.  A handle has entries only
behind a solve, so the refusals that need some (a cap below the source entries, a filter outside 1 .. 15 with every pool's bytes compared) and what
the call computes are in test_pool_carry_multi_gpu.py.
The count of pairs is refused before a handle is looked at (-5 on n alone), so the test of 2049 pairs hands in arrays of two handles."""
import ctypes as C
import os
import re

import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import PoolCarryC
from test_pool_carry_cpu import _kept, _loaded, _marked, _pairs_the_maps_refuse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS_MAX = 2048   # 65536 records of at most 32 per pair: 16 own and 16 carried


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def _handles(ws):
    return (C.c_void_p * len(ws))(*[w._h if w is not None else None for w in ws])


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _pooled(cfg="mini", seed=0, p=None, cap=8, fam=12, **kw):
    """an instance loaded, capacity and filter set, no solve: an empty pool"""
    w = _loaded(cfg, seed, p, **kw)
    assert w.setSolutionPool(cap) == 0 and w.setSolutionPoolFilter(fam) == 0
    return w


def test_the_exports_exist_and_bind(lib):
    hdr = open(os.path.join(ROOT, "include", "miqp_gpu.h")).read()
    for n in ("miqp_solver_pool_carry_multi", "miqp_gpu_pool_carry_multi_last"):
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS
        assert getattr(lib, n).argtypes
    assert lib.miqp_solver_pool_carry_multi.restype is C.c_int and lib.miqp_gpu_pool_carry_multi_last.restype is None
    assert len(lib.miqp_solver_pool_carry_multi.argtypes) == 8 and len(lib.miqp_gpu_pool_carry_multi_last.argtypes) == 2
    assert re.search(r"\bint\s+miqp_solver_pool_carry_multi\s*\(\s*miqp_solver_t\s*\*\s*const\s*\*\s*dsts\s*,\s*const\s+miqp_solver_t\s*\*\s*const\s*\*\s*srcs\s*,\s*int\s+n\s*,"
                     r"\s*int\s+shift\s*,\s*double\s+max_rel\s*,\s*miqp_pool_carry_c\s*\*\s*out\s*,\s*int\s+cap\s*,\s*int\s*\*\s*counts\s*\)", hdr)
    assert re.search(r"\bvoid\s+miqp_gpu_pool_carry_multi_last\s*\(\s*int\s*\*\s*rounds\s*,\s*int\s*\*\s*groups\s*\)", hdr)
    # what the call promises and refuses is said where it is declared; the single call no longer lists the pairs as out of scope
    for text in ("bit for bit", "a destination named twice", "the destination of one pair and the source of another", "2048 pairs", "takes no part"):
        assert text in hdr, text
    assert not re.search(r"Out of scope:\s*many", hdr)
    assert lib.miqp_gpu_pool_carry_size() == C.sizeof(PoolCarryC) == 32
    assert callable(P.carry_solution_pools) and callable(P.pool_carry_multi_last)
    assert P.carry_solution_pools is P.wrapper.carry_solution_pools and P.pool_carry_multi_last is P.wrapper.pool_carry_multi_last
    r, g = P.pool_carry_multi_last()
    assert isinstance(r, int) and isinstance(g, int)
    # the kernel file says the same, and keeps one copy of each kernel
    src = open(os.path.join(ROOT, "planner_miqp_amd", "csrc", "pool_carry.hip")).read()
    assert not re.search(r"Out of scope:\s*many", src)
    assert len(re.findall(r"__global__[^\n]*\bvoid\s+pool_shift_kernel\b", src)) == 1 and len(re.findall(r"__global__[^\n]*\bvoid\s+pool_carry_admit_kernel\b", src)) == 1


def test_refuses_before_a_device_is_asked_for(lib):
    f = lib.miqp_solver_pool_carry_multi
    base, others = _pairs_the_maps_refuse()
    s0, s1, d0, d1 = _pooled(p=base), _pooled(p=base.copy()), _pooled(p=base.copy()), _pooled(p=base.copy())
    ws = (s0, s1, d0, d1)
    out = _marked(32)
    counts = _ints(7, 7)
    hd, hs = _handles([d0, d1]), _handles([s0, s1])
    before = [_kept(w) for w in ws]
    # -1: NULL arrays, n <= 0, cap < 0, max_rel a NaN
    assert f(None, hs, 2, 1, -1.0, out, 16, counts) == -1 and f(hd, None, 2, 1, -1.0, out, 16, counts) == -1
    assert f(hd, hs, 2, 1, -1.0, None, 16, counts) == -1 and f(hd, hs, 2, 1, -1.0, out, 16, None) == -1
    assert f(hd, hs, 0, 1, -1.0, out, 16, counts) == -1 and f(hd, hs, -2, 1, -1.0, out, 16, counts) == -1
    assert f(hd, hs, 2, 1, -1.0, out, -1, counts) == -1
    assert f(hd, hs, 2, 1, float("nan"), out, 16, counts) == -1
    # -1: a NULL handle or one without an instance, on either side
    assert f(_handles([d0, None]), hs, 2, 1, -1.0, out, 16, counts) == -1 and f(hd, _handles([None, s1]), 2, 1, -1.0, out, 16, counts) == -1
    assert f(_handles([d0, P.CplexWrapper()]), hs, 2, 1, -1.0, out, 16, counts) == -1 and f(hd, _handles([s0, P.CplexWrapper()]), 2, 1, -1.0, out, 16, counts) == -1
    # -1: src == dst; a destination named twice; a handle that is the destination of one pair and the source of another
    assert f(hd, _handles([s0, d1]), 2, 1, -1.0, out, 16, counts) == -1
    assert f(_handles([d0, d0]), hs, 2, 1, -1.0, out, 16, counts) == -1
    assert f(hd, _handles([s0, d0]), 2, 1, -1.0, out, 16, counts) == -1 and f(hd, _handles([d1, s1]), 2, 1, -1.0, out, 16, counts) == -1
    # ... while one source may feed both destinations: nothing to carry here, so 0 and no device
    assert f(hd, _handles([s0, s0]), 2, 1, -1.0, out, 16, counts) == 0 and list(counts) == [0, 0]
    counts = _ints(7, 7)
    # -5: more than 2048 pairs, on the count alone (the arrays hold two handles and are not read)
    assert f(hd, hs, PAIRS_MAX + 1, 1, -1.0, out, 16, counts) == -5
    # -2: the shift outside 1 .. N - 2
    for bad in (0, -1, 5, 6, 100):
        assert f(hd, hs, 2, bad, -1.0, out, 16, counts) == -2, bad
    assert [_kept(w) for w in ws] == before
    # -2: a pair the single call refuses - no capacity, a filter outside 1 .. 15 - is named in ITS destination's last error, the other's stays
    assert d1.setSolutionPool(0) == 0 and f(hd, hs, 2, 1, -1.0, out, 16, counts) == -2 and d1.setSolutionPool(8) == 0
    assert "pair 1" in d1.lastError() and d0.lastError() == ""
    for fam in (0, 16, 16 + 12, 31):
        assert d0.setSolutionPoolFilter(fam) == 0 and f(hd, hs, 2, 1, -1.0, out, 16, counts) == -2, fam
        assert "pair 0" in d0.lastError() and "filter %d" % fam in d0.lastError()
    assert d0.setSolutionPoolFilter(12) == 0
    # (a call that nothing refuses clears every destination's last error)
    assert f(hd, hs, 2, 1, -1.0, out, 16, counts) == 0 and [d0.lastError(), d1.lastError()] == ["", ""] and list(counts) == [0, 0]
    counts = _ints(7, 7)
    # -2: what the maps refuse of a pair - the obstacles among the rest -, the reason in that destination's last error; the destination in front of
    # it keeps the last error it had.  The pairs are checked in order: behind a refused pair nothing is looked at
    assert d0.carrySolutionPool(s0, shift=0) == (-2, []) and d0.lastError() == ""
    for what, p, text in others:
        o = _pooled(p=p)
        assert f(_handles([d0, o]), hs, 2, 1, -1.0, out, 16, counts) == -2 and text in o.lastError() and d0.lastError() == "", (what, o.lastError())
        assert f(hd, _handles([s0, o]), 2, 1, -1.0, out, 16, counts) == -2 and text in d1.lastError() and d0.lastError() == "", (what, d1.lastError())
        assert f(_handles([o, d1]), hs, 2, 1, -1.0, out, 16, counts) == -2 and text in o.lastError(), (what, o.lastError())
        with pytest.raises(RuntimeError, match=text):
            P.carry_solution_pools([d0, o], [s0, s1])
        assert f(hd, hs, 2, 1, -1.0, out, 16, counts) == 0 and d1.lastError() == ""
        counts = _ints(7, 7)
    # -2: destinations of another shape although each pair is fine on its own (one car), with batch_layout's text on every destination; another device
    c_s, c_d = _pooled("mini1", 0), _pooled("mini1", 1)
    assert f(_handles([d0, c_d]), _handles([s0, c_s]), 2, 1, -1.0, out, 16, counts) == -2
    assert "share" in d0.lastError() and d0.lastError() == c_d.lastError()
    e0, e1 = _pooled(p=base.copy(), device=0), _pooled(p=base.copy(), device=1)
    assert f(_handles([e0, e1]), hs, 2, 1, -1.0, out, 16, counts) == -2 and "device" in e0.lastError()
    # nothing was written, nothing the handles keep has changed
    assert [(o.status, o.place) for o in out] == [(9, 9)] * 32 and list(counts) == [7, 7]
    assert [_kept(w)[:2] for w in ws] == [b[:2] for b in before]
    # ... and through the module function
    with pytest.raises(RuntimeError, match="share"):
        P.carry_solution_pools([d0, c_d], [s0, c_s])
    with pytest.raises(RuntimeError):
        P.carry_solution_pools([d0, d1], [s0, s1], shift=0)
    with pytest.raises(RuntimeError):
        P.carry_solution_pools([d0, d1], [s0, s1], max_rel=float("nan"))
    with pytest.raises(RuntimeError):
        P.carry_solution_pools([d0, d0], [s0, s1])
    with pytest.raises(ValueError):
        P.carry_solution_pools([d0, d1], [s0])


def test_pairs_without_pools_return_0_without_a_device(lib):
    """no source keeps an entry - no solve - so no pair takes part: the call returns 0, every count 0, nothing written to `out`, a last error
    cleared as the single call clears it; none of it needs a device"""
    f = lib.miqp_solver_pool_carry_multi
    ss = [_pooled(seed=k) for k in range(3)]
    ds = [_pooled(seed=k, cap=c, fam=m) for k, c, m in ((0, 8, 12), (1, 1, 4), (2, 16, 15))]
    # a last error from an earlier refusal
    assert f(_handles(ds), _handles(ss), 3, 0, -1.0, _marked(48), 16, _ints(7, 7, 7)) == -2
    assert ds[1].carrySolutionPool(_loaded("mini1", 0)) == (-2, []) and ds[1].lastError()
    before = [_kept(w)[:2] for w in ss + ds]
    out = _marked(48)
    counts = _ints(7, 7, 7)
    assert f(_handles(ds), _handles(ss), 3, 1, 0.5, out, 16, counts) == 0
    assert list(counts) == [0, 0, 0] and [(o.status, o.place) for o in out] == [(9, 9)] * 48
    assert [_kept(w)[:2] for w in ss + ds] == before
    assert [w.lastError() for w in ds] == [""] * 3
    # cap 0 is enough when no source keeps anything
    assert f(_handles(ds), _handles(ss), 3, 1, -1.0, out, 0, counts) == 0
    assert P.carry_solution_pools(ds, ss) == [(0, [])] * 3
    assert P.carry_solution_pools(ds, [ss[0]] * 3, shift=2, max_rel=0.0) == [(0, [])] * 3

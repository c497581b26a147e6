"""improve_solution_pools - the pools of MANY wrappers hill-climbed in one device call (miqp_solver_pool_improve_multi) - against the
single-handle call improveSolutionPool, which tests/test_pool_improve_gpu.py pins against its host replay.

Single solves are bit-reproducible (test_pool_filter_gpu.py::test_reproducible, test_pool_improve_gpu.py::test_the_solve_is_untouched), so every
comparison solves TWIN sets of fresh wrappers: set one gets miqp_solver_pool_improve per wrapper, set two ONE improve_solution_pools call.  Compared
bit for bit and per wrapper: moved, before, after, moves, status, the final decision bytes of every entry, the found objectives, last_timing
out[2 .. 5] and whether lastError() is empty.
All tests here need a real MI355X: run with  python -m pytest tests/test_pool_improve_multi_gpu.py -m gpu -s."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import PoolImproveC
from test_pool_filter_gpu import FILTER, _as_found, _signatures
from test_pool_filter_gpu import _params as _filter_params
from test_pool_improve_gpu import WRAP2_CFG, _same_solve

pytestmark = pytest.mark.gpu

NB_MAX = 8192   # results of a slice
_PARAMS = {}


def _cfg4(seed):
    """shared with the filter and climb suites, and left unchanged"""
    return _filter_params("cfg4s%d" % seed)


def _other(name, seed):
    """c2n6e2pent's configuration (as helpers.node_instance makes it) and the 76-site shape (2, 8, 32, 2, 6), under further seeds"""
    if (name, seed) not in _PARAMS:
        if name == "wrap2":
            _PARAMS[(name, seed)] = synthetic.generate(WRAP2_CFG, seed, gap=1e-4)
        else:
            cfg, _, tweaks = H.NODE_SHAPES[name]
            p = synthetic.generate(cfg, seed, gap=1e-7, max_time=30)
            H.tweak_instance(p, **tweaks)
            _PARAMS[(name, seed)] = p
    return _PARAMS[(name, seed)]


def _make(spec):
    """fresh wrappers, solved one by one: spec is a list of (parameters, capacity, filter); capacity 0: the pool stays off"""
    ws = []
    for p, cap, fam in spec:
        w = P.CplexWrapper(); w.resetParameters(p)
        if cap:
            assert w.setSolutionPool(cap) == 0 and w.setSolutionPoolFilter(fam) == 0
        assert w.callCplex() == P.OptimizationStatus.SUCCESS
        assert (w.solutionPoolCount() >= 1) == bool(cap)
        ws.append(w)
    return ws


def _timing(w):
    t = (C.c_double * 6)()
    assert w._L.miqp_solver_last_timing(w._h, t) == 0
    return list(t)


def _pool(w):
    n = w.solutionPoolCount()
    return dict(n=n, found=w.solutionPoolFound().tobytes(), dec=[w.solutionPoolFoundDecisions(k).tobytes() for k in range(n)])


def _state(w, answer):
    moved, before, after, moves, status = answer
    t = _timing(w)
    s = _pool(w)
    s.update(moved=moved, before=before, after=after, moves=moves, status=status, timing=t[2:6], device_ms=1e3 * t[1], call_ms=1e3 * t[0], quiet=w.lastError() == "")
    return s


def _single(w, passes, cap=None):
    """miqp_solver_pool_improve of one wrapper, through the C ABI so that `cap` can be given"""
    n = w.solutionPoolCount()
    c = max(n, 1) if cap is None else cap
    out = (PoolImproveC * c)()
    rc = int(w._L.miqp_solver_pool_improve(w._h, passes, out, c))
    assert rc >= 0, rc
    a = np.frombuffer(out, dtype=np.dtype([("before", "<f8"), ("after", "<f8"), ("moves", "<i4"), ("status", "<i4")]), count=min(n, c))
    return _state(w, (rc, a["before"].copy(), a["after"].copy(), a["moves"].copy(), a["status"].copy()))


def _same(a, b, what):
    assert a["moved"] == b["moved"] and a["n"] == b["n"], (what, a["moved"], b["moved"], a["n"], b["n"])
    for n in ("before", "after", "moves", "status"):
        assert a[n].dtype == b[n].dtype and a[n].tobytes() == b[n].tobytes(), (what, n, list(a[n]), list(b[n]))
    assert a["found"] == b["found"], what
    for k in range(a["n"]):
        assert a["dec"][k] == b["dec"][k], (what, k)
    assert a["timing"] == b["timing"], (what, a["timing"], b["timing"])
    assert a["quiet"] == b["quiet"], what


def _twins(spec, passes, cap=None, what=""):
    """set one through the single call, set two through ONE multi call; both lists of states (wrappers whose pool is off: only the multi side)"""
    one, two = _make(spec), _make(spec)
    pre = [dict(_pool(b), timing=_timing(b)) for b in two]
    for a, b in zip(one, pre):
        assert _pool(a) == {k: b[k] for k in ("n", "found", "dec")}, what   # (the twin solves are one solve)
    single = [_single(w, passes, cap) if w.solutionPoolCount() else None for w in one]
    multi = [_state(w, r) for w, r in zip(two, P.improve_solution_pools(two, max_passes=passes, cap=cap))]
    for k, (s, m) in enumerate(zip(single, multi)):
        if s is None:   # a wrapper that kept nothing is left alone: empty arrays, and last_timing is still that of its solve
            assert m["n"] == 0 and m["moved"] == 0 and all(len(m[n]) == 0 for n in ("before", "after", "moves", "status")), (what, k)
            assert _timing(two[k]) == pre[k]["timing"], (what, k)
            continue
        print("MULTI %s passes %d wrapper %d: %d entries, %d moved, passes %d, neighbours %d, iterations %d, still moving %d | call: device %.1f ms of %.1f ms%s"
              % (what, passes, k, m["n"], m["moved"], m["timing"][0], m["timing"][1], m["timing"][2], m["timing"][3], m["device_ms"], m["call_ms"],
                 " | alone: device %.1f ms of %.1f ms" % (s["device_ms"], s["call_ms"])))
        _same(s, m, (what, passes, k))
    return single, multi, two, pre


MIXED = [(1, FILTER), (4, FILTER), (9, FILTER), (7, FILTER), (0, P.POOL_BY_CAR_CAR)]   # cfg4 seeds and their filters: the filters differ within the call


def _mixed_spec():
    return [(_cfg4(seed), 8, fam) for seed, fam in MIXED]


@pytest.mark.parametrize("passes", [1, 2, 8])
def test_equals_the_single_call(passes):
    """cfg4 seeds 1, 4, 9 and 7 under filter 12 and seed 0 under filter 8 in one call.  At 8 passes at least two wrappers move, and they do not all
    finish in the same number of passes (seed 1 three passes, seed 4 four, seed 9 more): a finished handle stays finished -
    contributes no nodes, keeps its figures - while the others go on"""
    single, multi, ws, pre = _twins(_mixed_spec(), passes, what="mixed")
    assert all(m["timing"][0] <= passes for m in multi)
    if passes == 8:
        assert sum(1 for m in multi if m["moved"] > 0) >= 2, [m["moved"] for m in multi]
        assert len({m["timing"][0] for m in multi}) >= 2, [m["timing"][0] for m in multi]


def test_order_and_cap():
    """the same wrappers in reverse order with a wrapper whose pool is off in the middle: the same per-wrapper answers; cap = 2 is the single call at cap = 2"""
    spec = _mixed_spec()[::-1]
    spec.insert(2, (_cfg4(2), 0, 0))
    single, multi, ws, pre = _twins(spec, 8, what="reversed")
    assert multi[2]["n"] == 0 and ws[2].solutionPoolCount() == 0
    fw = _make(_mixed_spec())   # what a wrapper gets does not depend on its place in the call or on its companions: a third set, in forward order
    forward = [_state(w, r) for w, r in zip(fw, P.improve_solution_pools(fw, max_passes=8))]
    for a, b in zip(forward[::-1], multi[:2] + multi[3:]):
        _same(a, b, "order")
    single, multi, ws, pre = _twins(_mixed_spec(), 8, cap=2, what="cap 2")
    assert all(len(m["before"]) == min(m["n"], 2) for m in multi) and any(m["n"] > 2 for m in multi)


OTHER_SEEDS = {"c2n6e2pent": (0, 6, 7), "wrap2": (3, 10, 11)}   # (c2n6e2pent: the first three seeds whose tweaked instance has a solution)


@pytest.mark.parametrize("name,fam", [("c2n6e2pent", FILTER), ("wrap2", 1)], ids=["c2n6e2pent", "wrap2"])
def test_other_shapes(name, fam):
    """three DIFFERENT instances of c2n6e2pent's shape, and of the 76-site shape (2, 8, 32, 2, 6) seeds 3, 10 and 11 under filter 1, whose moves cross
    lane 63 (test_pool_improve_gpu.py): a kernel that reads another handle's record, filter or tables does not pass"""
    spec = [(_other(name, seed), 8, fam) for seed in OTHER_SEEDS[name]]
    single, multi, ws, pre = _twins(spec, 8, what=name)
    assert sum(m["timing"][1] for m in multi) > 0, name   # (there were neighbours to solve)
    assert len({m["dec"][0] for m in multi}) == 3, name   # (the instances differ)


SLICE_SEEDS = [9, 15, 11, 2, 14, 5, 9, 9, 9]   # cfg4 at capacity 16; seed 9 has 1295 neighbours in its first pass


@pytest.mark.parametrize("passes", [1, 8])
def test_slices(passes):
    """more than 8192 neighbours in the first pass: the results of a pass are kept a slice at a time"""
    spec = [(_cfg4(seed), 16, FILTER) for seed in SLICE_SEEDS]
    single, multi, ws, pre = _twins(spec, passes, what="slices")
    if passes == 1:
        first = [m["timing"][1] for m in multi]   # out[3] behind max_passes = 1: the neighbours of the first pass
        assert first[0] == first[6] == 1295 and sum(first) > NB_MAX, first
        # per entry: the kept moves of the record as found, those of an entry whose own QP is not feasible (never expanded) set to 0
        counts = []
        for w, m, found in zip(ws, multi, pre):
            d = (C.c_int * 6)(); assert w._L.miqp_solver_get_dims(w._h, d) == 0
            for k in range(m["n"]):
                counts.append(len(P.pool_moves(d[0], d[1], d[4], FILTER, np.frombuffer(found["dec"][k], dtype=np.int8))) if m["status"][k] == 0 else 0)
        assert sum(counts) == sum(first), (sum(counts), sum(first))
        plan = P.pool_improve_plan(counts)
        print("MULTI slices: first-pass neighbours per wrapper %s, total %d, slices at entries %s" % (first, sum(first), plan))
        assert len(plan) - 1 >= 2, plan


def test_stream():
    """six cfg4 instances drained with two in flight, capacity 8, filter 12; the climb of all of them in one call, then the refinement in one call"""
    ws = []
    for k in range(6):
        w = P.CplexWrapper(); w.resetParameters(_cfg4(k))
        assert w.setSolutionPool(8) == 0 and w.setSolutionPoolFilter(FILTER) == 0
        ws.append(w)
    sts = P.solve_batch(ws, inflight=2)
    assert all(st == P.OptimizationStatus.SUCCESS for st in sts), sts
    found = [_as_found(w, sts[k]) for k, w in enumerate(ws)]
    res = P.improve_solution_pools(ws)
    alive = []
    for k, (w, s, (moved, before, after, moves, status)) in enumerate(zip(ws, found, res)):
        assert len(before) == s["n"] == w.solutionPoolCount() >= 1, k
        assert (after <= before).all() and moved == int((moves > 0).sum()), k
        now = dict(s, dec=[w.solutionPoolFoundDecisions(j) for j in range(s["n"])])
        assert _signatures(now) == _signatures(s), k   # every entry stayed in its class
        alive.append({np.float64(a).tobytes() for a, x in zip(after, status) if x == 0})
        print("MULTI stream %d: %d entries, %d moved, before %s after %s" % (k, s["n"], moved, list(before), list(after)))
    refined = P.solve_solution_pools(ws)
    for k, (w, (st, obj, viol, it, route)) in enumerate(zip(ws, refined)):
        fnd = w.solutionPoolFound()
        assert len(obj) == w.solutionPoolCount() == len(fnd) >= 1, k
        for j in range(len(obj)):
            rc, rec = w.solutionPoolRecord(j)
            if np.float64(fnd[j]).tobytes() not in alive[k]:
                continue   # (an entry the climb left as it was found: not feasible at the tight tolerance)
            assert st[j] == 0 and rc == 0, (k, j, st[j], rc)
            assert obj[j] <= fnd[j] * (1 + 1e-7), (k, j, obj[j], fnd[j])
            cert = w.certify(rec)
            assert cert.status == 0 and cert.max_violation < 1e-5, (k, j, cert)


def test_refusals_on_a_device():
    """a handle that kept entries without a filter: -2, named in its last error, and every pool of the call has the bytes it had; a wrapper outside
    the call is untouched; a solve behind a climb equals a fresh solve"""
    a, b, c = _make([(_cfg4(1), 8, FILTER), (_cfg4(4), 8, 0), (_cfg4(1), 8, FILTER)])
    before = [_pool(w) for w in (a, b, c)]
    out = (PoolImproveC * 16)()
    for o in out:
        o.status = 9
    counts = (C.c_int * 2)(7, 7)
    rc = a._L.miqp_solver_pool_improve_multi((C.c_void_p * 2)(a._h, b._h), 2, 8, out, 8, counts)
    assert rc == -2 and "handle 1" in b.lastError() and "filter" in b.lastError(), (rc, b.lastError())
    assert [o.status for o in out] == [9] * 16 and list(counts) == [7, 7]
    assert [_pool(w) for w in (a, b, c)] == before
    with pytest.raises(RuntimeError, match="handle 0 of the call kept entries under filter 0"):
        P.improve_solution_pools([b, a])
    with pytest.raises(RuntimeError, match="handle 1 of the call kept entries under filter 0"):   # (the text of the handle that was refused, not of the first)
        P.improve_solution_pools([a, b])
    assert [_pool(w) for w in (a, b, c)] == before
    fresh = _as_found(c, P.OptimizationStatus.SUCCESS)
    res = P.improve_solution_pools([a])
    assert res[0][0] >= 1 and _pool(a) != before[0]   # (entry 1 of seed 1 moves)
    assert _pool(c) == before[2]
    _same_solve(fresh, _as_found(a, a.callCplex()), "a solve behind the climb of many")


def test_reproducible():
    """two fresh sets through the multi call agree byte for byte"""
    runs = []
    for _ in range(2):
        ws = _make(_mixed_spec())
        runs.append([_state(w, r) for w, r in zip(ws, P.improve_solution_pools(ws, max_passes=8))])
    for k, (x, y) in enumerate(zip(*runs)):
        _same(x, y, ("reproducible", k))

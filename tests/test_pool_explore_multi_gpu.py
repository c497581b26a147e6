"""The free places of the solution pools of many handles filled in one device call (explore_solution_pools).

The reference of the call is the loop of single calls: set A, fresh wrappers, goes through exploreSolutionPool wrapper by wrapper; set B, their twins
(single solves are bit-reproducible), through ONE explore_solution_pools call.  Per wrapper both sides are compared bit for bit: the count and the
dicts (`solves` of the settled mode included), solutionPoolCount(), solutionPoolFound(), every solutionPoolFoundDecisions(k), last_timing[2 .. 5] and
what lastError() says.  The single calls are pinned against host replays by test_pool_explore_gpu.py, test_pool_label_gpu.py and
test_pool_settle_gpu.py, which run the same kernels with one handle.
Instances: those of test_pool_explore_gpu.py (_params and FILTER of test_pool_filter_gpu: filter 12, gap as there).  Every run is made once per
module and shared; a test that goes on with a run's wrappers makes its own.
All tests here need a real MI355X: run with  python -m pytest tests/test_pool_explore_multi_gpu.py -m gpu -s."""
import ctypes as C

import numpy as np
import pytest

import planner_miqp_amd as P
from test_node_qp_gpu import _bytes
from test_pool_filter_gpu import FILTER, _params

pytestmark = pytest.mark.gpu

MODES = ["plain", "distinct", "settled"]
NOTHING = ("cfg4s3", 16, FILTER, False)   # a wrapper of the shape that is loaded and never solved: it kept nothing
# (name, capacity, filter, solved)
SET1 = [("cfg4s7", 16, FILTER, True), ("cfg4s12", 16, FILTER, True), ("cfg4s1", 8, FILTER, True), ("cfg4s9", 16, FILTER, True)]   # capacities differ; seed 9 is full
SET1 = SET1[:2] + [SET1[3], SET1[2]]   # ... and sits in the middle: seeds 7, 12, 9, 1
SET2 = [SET1[3], SET1[2], NOTHING, SET1[1], SET1[0]]   # the reverse, with a wrapper that kept nothing in the middle
SET3 = SET1 + [("cfg4s10", 16, FILTER, True), ("cfg4s5", 16, FILTER, True)]   # handles that stop in different passes
SET4A = [("c2n6e2pent", 8, 12, True), ("c2n6e2pent", 8, 4, True), ("c2n6e2pent", 8, 8, True)]   # one shape under three filters
SET4B = [("wrap", 8, 12, True), ("wrap", 8, 4, True), ("wrap", 8, 8, True)]   # 76 sites: the lane loop wraps
SET5 = [("cfg4s%d" % s, 16, FILTER, True) for s in (14, 11, 15, 2, 8)]   # more than 8192 neighbours in pass 1: two slices
_RUNS = {}


def _wrapper(name, cap, fam, solved):
    w = P.CplexWrapper(); w.resetParameters(_params(name))
    assert w.setSolutionPool(cap) == 0 and w.setSolutionPoolFilter(fam) == 0
    if solved:
        assert w.callCplex() == P.OptimizationStatus.SUCCESS and w.solutionPoolCount() >= 1, (name, cap, fam)
    else:
        assert w._push_inputs() == 0 and w.solutionPoolCount() == 0
    return w


def _timing(w):
    t = (C.c_double * 6)()
    assert w._L.miqp_solver_last_timing(w._h, t) == 0
    return list(t)


def _pool(w):
    """the pool of a wrapper, as bytes"""
    n = w.solutionPoolCount()
    return (n, np.asarray(w.solutionPoolFound(), dtype=np.float64).tobytes(), [w.solutionPoolFoundDecisions(k).tobytes() for k in range(n)])


def _snap(w, rc, added, n0):
    return dict(rc=rc, added=added, n0=n0, pool=_pool(w), timing=_timing(w)[2:6], err=w.lastError())


def _kw(mode, passes, max_rel):
    return dict(max_passes=passes, max_rel=max_rel, distinct=mode == "distinct", settled=mode == "settled")


def _singles(spec, mode, passes, max_rel):
    """set A: a fresh wrapper per item through its own exploreSolutionPool.  The single call of a wrapper does not depend on the set it stands in,
    so the sets share these; the solves of the missing ones run first, then their calls (a solve and a pool call size the device context
    differently: alternating them rebuilds it every time)"""
    todo = [(item, _wrapper(*item)) for item in dict.fromkeys(spec) if (item, mode, passes, max_rel) not in _RUNS]
    for item, w in todo:
        n0 = w.solutionPoolCount()
        rc, added = w.exploreSolutionPool(**_kw(mode, passes, max_rel))
        _RUNS[(item, mode, passes, max_rel)] = _snap(w, rc, added, n0)
    return [_RUNS[(item, mode, passes, max_rel)] for item in spec]


def _multi(spec, mode, passes, max_rel, keep=True, ws=None):
    """set B: fresh wrappers of `spec` (ws: made by the caller) through ONE explore_solution_pools call, and what every wrapper shows behind it"""
    key = (tuple(spec), mode, passes, max_rel)
    if keep and key in _RUNS:
        return _RUNS[key]
    ws = ws if ws is not None else [_wrapper(*s) for s in spec]
    n0 = [w.solutionPoolCount() for w in ws]
    res = P.explore_solution_pools(ws, **_kw(mode, passes, max_rel))
    r = dict(ws=ws if not keep else None, snaps=[_snap(w, rc, added, k) for w, (rc, added), k in zip(ws, res, n0)])
    if keep:
        _RUNS[key] = r
    return r


def _same(spec, mode, passes, max_rel, adding=2):
    """set A against set B, wrapper by wrapper; returns set A's snapshots.  adding: on how many handles set A - the single calls, not the code under
    test - has to add an entry for the comparison to say something"""
    key = (tuple(spec), mode, passes, max_rel)
    ws = [_wrapper(*s) for s in spec] if key not in _RUNS else None   # (set B's solves in front of set A's calls: see _singles)
    a = _singles(spec, mode, passes, max_rel)
    b = _multi(spec, mode, passes, max_rel, ws=ws)["snaps"]
    print("MULTI %-8s passes %d max_rel %4g | %s" % (mode, passes, max_rel, " | ".join(
        "%s/%d f%d: %d -> %d, passes %d, solves %d" % (s[0], s[1], s[2], x["n0"], x["pool"][0], x["timing"][0], x["timing"][1]) for s, x in zip(spec, a))))
    assert sum(1 for x in a if x["rc"] >= 1) >= adding, [x["rc"] for x in a]
    for h, (x, y) in enumerate(zip(a, b)):
        what = (spec[h], mode, passes, max_rel)
        assert x["rc"] >= 0 and x["rc"] == y["rc"], (what, x["rc"], y["rc"], y["err"])
        assert x["added"] == y["added"], what   # (ints, and floats that compare equal only bit for bit - no NaN among the objectives)
        assert all(np.float64(p["objective"]).tobytes() == np.float64(q["objective"]).tobytes() for p, q in zip(x["added"], y["added"])), what
        assert all(("solves" in p) == (mode == "settled") for p in y["added"]), what
        assert x["pool"][0] == y["pool"][0] == x["n0"] + x["rc"], what
        assert x["pool"] == y["pool"], what
        assert x["timing"] == y["timing"], (what, x["timing"], y["timing"])
        assert x["err"] == y["err"], (what, x["err"], y["err"])
    return a


def _adding(mode):
    """Cases 1 and 2 are the seeds 7, 12, 1 and 9.  The plain and the distinct call add on seeds 7, 12 and 1; the settled call adds on seed 12 alone
    (test_pool_settle_gpu.py and DESIGN.md 6j: seeds 7 and 1 settle back onto entries the pool holds, seed 9 is full), which is why seed 12 is in
    every set - so there one adding handle is all these four seeds can give; case 3 has the settled call add on three"""
    return 1 if mode == "settled" else 2


def _as_found(spec):
    """per item a fresh solve of a wrapper of its kind: its pool and solution as bytes, and what the refinement leaves of the pool as found (L0).
    The solves of the missing ones first, then one refinement of all of them"""
    todo = [(item, _wrapper(*item)) for item in dict.fromkeys(spec) if ("found", item) not in _RUNS]
    for item, w in todo:
        p = w.getSolutionProperties()
        _RUNS[("found", item)] = dict(pool=_pool(w), bytes=_bytes(w.getRawResults(), p.objective), nodes=p.nodes)
    if todo:
        P.solve_solution_pools([w for item, w in todo])
    for item, w in todo:
        _RUNS[("found", item)]["left"] = w.solutionPoolCount()
    return [_RUNS[("found", item)] for item in spec]


# ------------------------------------------------------------------------------------------------------------------------------ 1, 2, 6.
@pytest.mark.parametrize("max_rel", [-1.0, 0.5])
@pytest.mark.parametrize("passes", [1, 4])
@pytest.mark.parametrize("mode", MODES)
def test_capacities_differ_and_a_full_pool_in_the_middle(mode, passes, max_rel):
    a = _same(SET1, mode, passes, max_rel, _adding(mode))
    assert a[2]["rc"] == 0 and a[2]["n0"] == 16   # (seed 9 is full: it takes no part)
    assert a[3]["pool"][0] <= 8
    if mode == "settled" and passes == 4:
        assert all("solves" in p and 1 <= p["solves"] <= P.pool_settle_passes() for x in a for p in x["added"])


@pytest.mark.parametrize("max_rel", [-1.0, 0.5])
@pytest.mark.parametrize("passes", [1, 4])
@pytest.mark.parametrize("mode", MODES)
def test_in_reverse_with_a_wrapper_that_kept_nothing(mode, passes, max_rel):
    a = _same(SET2, mode, passes, max_rel, _adding(mode))
    assert a[2]["rc"] == 0 and a[2]["pool"][0] == 0 and a[2]["err"] == ""
    # the order of the handles changes no handle's answer: the same bits as in the set of case 1
    fwd = _multi(SET1, mode, passes, max_rel)["snaps"]
    rev = _multi(SET2, mode, passes, max_rel)["snaps"]
    for k, j in ((0, 4), (1, 3), (2, 1), (3, 0)):
        assert fwd[k] == rev[j], (SET1[k], mode, passes, max_rel)


def test_the_last_pass_still_added_is_said_per_handle():
    """1 pass, plain: seeds 7 and 12 add in the last allowed pass; with places still free the handle says so, in the single call's words"""
    a = _same(SET1, "plain", 1, 0.5)
    b = _multi(SET1, "plain", 1, 0.5)["snaps"]
    said = 0
    for x, y in zip(a, b):
        assert x["timing"][3] == y["timing"][3]
        if x["err"]:
            assert y["err"].startswith("miqp_solver_pool_explore: the last of 1 passes still added") and y["timing"][3] == 1
            said += 1
    assert said >= 1


# ------------------------------------------------------------------------------------------------------------------------------ 3.
@pytest.mark.parametrize("mode", ["distinct", "settled"])
def test_handles_that_stop_in_different_passes(mode):
    a = _same(SET3, mode, 4, -1.0)
    took_part = [x for s, x in zip(SET3, a) if 0 < x["n0"] < s[1]]   # (the timing of the full pool's handle is still its solve's)
    ran = sorted({int(x["timing"][0]) for x in took_part})
    print("MULTI %s: passes per handle %s" % (mode, [int(x["timing"][0]) for x in took_part]))
    assert len(ran) >= 3, ran


# ------------------------------------------------------------------------------------------------------------------------------ 4.
@pytest.mark.parametrize("spec", [SET4A, SET4B], ids=["c2n6e2pent", "wrap"])
@pytest.mark.parametrize("mode", MODES)
def test_filters_differ(mode, spec):
    a = _same(spec, mode, 4, -1.0, 2 if spec is SET4A or mode == "plain" else 0)
    assert all(x["timing"][0] >= 1 for x in a), [x["timing"] for x in a]   # every filter has jumps here


# ------------------------------------------------------------------------------------------------------------------------------ 5.
def _pass1_totals(spec):
    """per wrapper the jumps of its pool as found (0 for a full pool): pool_jumps on the host"""
    if ("totals", tuple(spec)) in _RUNS:
        return _RUNS[("totals", tuple(spec))]
    tot = _RUNS[("totals", tuple(spec))] = []
    for name, cap, fam, solved in spec:
        w = _wrapper(name, cap, fam, solved)
        d = (C.c_int * 6)()
        assert w._L.miqp_solver_get_dims(w._h, d) == 0
        n = w.solutionPoolCount()
        tot.append(0 if n >= cap else sum(len(P.pool_jumps(d[0], d[1], d[4], d[5], fam, w.solutionPoolFoundDecisions(k))) for k in range(n)))
    return tot


def test_the_five_seeds_need_two_slices():
    tot = _pass1_totals(SET5)
    first = P.pool_explore_plan(tot)
    print("MULTI slices: pass-1 neighbours %s = %d, slices %s" % (tot, sum(tot), first))
    assert sum(tot) > 8192 and len(first) - 1 >= 2


@pytest.mark.parametrize("passes", [1, 4])
@pytest.mark.parametrize("mode", ["plain", "settled"])
def test_more_than_one_slice(mode, passes):
    a = _same(SET5, mode, passes, -1.0)
    assert sum(x["rc"] for x in a) >= 5
    if mode == "plain" and passes == 1:   # the plain call's solves of pass 1 are the neighbours the plan is asked about, and the call ran its slices
        tot = [int(x["timing"][1]) for x in a]
        assert tot == _pass1_totals(SET5)
        ws = [_wrapper(*s) for s in SET5]
        P.explore_solution_pools(ws, max_passes=1)
        assert P.pool_explore_multi_last() == (1, len(P.pool_explore_plan(tot)) - 1)


# ------------------------------------------------------------------------------------------------------------------------------ 7.
@pytest.mark.parametrize("mode", MODES)
def test_behind_the_call(mode):
    spec = SET1
    # (every solve of the test in front of its pool calls: a solve and a pool call size the device context differently)
    outside = _wrapper("cfg4s12", 16, FILTER, True)
    out0 = _pool(outside), _timing(outside), outside.lastError()
    ws = [_wrapper(*s) for s in spec]
    twins = [_wrapper(*s) for s in spec] if (tuple(spec), mode, 4, -1.0) not in _RUNS else None
    found = _as_found(spec)
    a = _singles(spec, mode, 4, -1.0)
    b = _multi(spec, mode, 4, -1.0, keep=False, ws=ws)
    assert (_pool(outside), _timing(outside), outside.lastError()) == out0   # a wrapper outside the call is untouched
    # two fresh B sets agree byte for byte
    assert b["snaps"] == _multi(spec, mode, 4, -1.0, ws=twins)["snaps"]
    l0 = [f["left"] for f in found]
    n_behind = [w.solutionPoolCount() for w in ws]
    P.improve_solution_pools(ws) if mode != "settled" else None   # (the climb moves labels: the settled invariant is about the pool as the call left it)
    res = P.solve_solution_pools(ws)
    certified = 0
    for h, (w, (st, obj, viol, it, route)) in enumerate(zip(ws, res)):
        assert 1 <= len(obj) == w.solutionPoolCount() <= n_behind[h]
        if mode == "settled":   # the refinement leaves exactly L0 + added
            assert w.solutionPoolCount() == l0[h] + a[h]["rc"], (spec[h], l0[h], a[h]["rc"], w.solutionPoolCount())
        for k in range(len(obj)):
            rc, rec = w.solutionPoolRecord(k)
            assert (rc == 0) == (st[k] == 0), (spec[h], k, rc, st[k])
            if rc == 0:
                cert = w.certify(rec)
                assert cert.status == 0 and cert.max_violation < 1e-5, (spec[h], k, cert)
                certified += 1
    assert certified >= len(spec)
    if mode == "settled":   # ... and the climb runs behind the call as well
        assert all(r[0] >= 0 for r in P.improve_solution_pools(ws))
    # a solve behind the call equals a fresh one
    for s, w, f in zip(spec, ws, found):
        assert w.callCplex() == P.OptimizationStatus.SUCCESS
        pw = w.getSolutionProperties()
        assert _pool(w) == f["pool"] and _bytes(w.getRawResults(), pw.objective) == f["bytes"] and pw.nodes == f["nodes"], s


# ------------------------------------------------------------------------------------------------------------------------------ 8.
def test_refusals_that_need_a_pool_leave_every_pool_alone():
    ws = [_wrapper("cfg4s7", 16, FILTER, True), _wrapper("cfg4s12", 16, 0, True), _wrapper("cfg4s1", 8, FILTER, True)]
    timing = _wrapper("cfg4s12", 16, 16 | FILTER, True)   # the timing bit: outside 1 .. 15
    region = _wrapper("cfg4s12", 16, 3, True)             # in 1 .. 15, with neither the obstacle nor the car/car family
    before = [_pool(w) for w in ws + [timing, region]]
    assert all(0 < p[0] for p in before)
    for mode in MODES:
        with pytest.raises(RuntimeError, match=r"\(-2\).*handle 1 of the call.*filter 0"):
            P.explore_solution_pools(ws, **_kw(mode, 4, -1.0))
        assert "handle 1" in ws[1].lastError()
    for bad, fam in ((timing, 28), (region, 3)):
        if bad.solutionPoolCount() < 16:
            with pytest.raises(RuntimeError, match=r"\(-2\).*handle 2 of the call.*filter %d" % fam):
                P.explore_solution_pools([ws[0], ws[2], bad])
    # a cap below the free places of a handle that takes part: -2, nothing written
    L = P.load_library()
    two = [ws[0], ws[2]]
    free = max(16 - ws[0].solutionPoolCount(), 8 - ws[2].solutionPoolCount())
    assert free >= 1
    out = (P.PoolExploreC * (2 * 16))()
    for o in out:
        o.parent = 9
    counts = (C.c_int * 2)(7, 7)
    hs = (C.c_void_p * 2)(*[w._h for w in two])
    assert L.miqp_solver_pool_explore_multi(hs, 2, 0, 4, -1.0, out, free - 1, counts) == -2
    assert [o.parent for o in out] == [9] * 32 and list(counts) == [7, 7]
    assert [_pool(w) for w in ws + [timing, region]] == before
    # ... and the same handles with the cap they need
    assert L.miqp_solver_pool_explore_multi(hs, 2, 0, 4, -1.0, out, free, counts) >= 1
    assert [out[h * free + k].parent for h in range(2) for k in range(counts[h])] != [9] * sum(counts)

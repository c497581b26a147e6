"""solve_fixed_multi and solve_solution_pools - the fix records and the solution pools of MANY wrappers in one device call - against the single-handle
calls they stand for, byte by byte.

The node kernels take nodes of several instances in one launch in every round of the branch and bound; what is new here is the host runner that numbers
the nodes of a call handle-major, the collect kernel that takes the constant cost per node from its instance and reduces one minimum per handle, and
the common Layout the handles of a call run under.  So every test holds one call over several wrappers against solveFixedBatch / solveSolutionPool
on TWIN wrappers (fresh ones on the same parameters), one call each: the five arrays, best, and every byte of every record.  The records of a
wrapper are the incumbent of a device solve of its instance and the refined records of that solve's pool - computed once per instance and left
unchanged.  All tests here need a real MI355X: run with  python -m pytest tests/test_fixed_multi_gpu.py -m gpu."""
import ctypes as C
import time

import numpy as np
import pytest

import helpers as H
import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import FixedResultC, RawResults
from test_node_qp_gpu import _bytes

pytestmark = pytest.mark.gpu

BIN = H.BIN_FIELDS + ["car2car_collision"]
ARRAYS = ("status", "objective", "violation", "iterations", "route")
_PARAMS, _RECORDS, _SINGLE = {}, {}, {}


def _params(key):
    """parameters of (config, seed, gap) - shared and left unchanged"""
    if key not in _PARAMS:
        cfg, seed, gap = key
        _PARAMS[key] = synthetic.generate(cfg, seed, gap=gap)
    return _PARAMS[key]


def _wrapper(p, cap=0):
    w = P.CplexWrapper(); w.resetParameters(p)
    assert w.setSolutionPool(cap) == 0
    return w


def _records_of(tag, p, cap=4):
    """[incumbent] + the refined records of the pool of one device solve of p (at least one record; the pool's entry 0 carries the incumbent's
    binaries, so the list holds one QP twice under two records: a tie for `best`)"""
    if tag not in _RECORDS:
        t0 = time.perf_counter()
        w = _wrapper(p, cap)
        assert w.callCplex() == P.OptimizationStatus.SUCCESS, tag
        recs = [w.getRawResults()]
        st = w.solveSolutionPool()[0]
        for k in range(len(st)):
            rc, r = w.solutionPoolRecord(k)
            assert rc == 0, (tag, k, rc)
            recs.append(r)
        _RECORDS[tag] = recs
        print("FIXEDMULTI records of %s: %d (%.2f s)" % (tag, len(recs), time.perf_counter() - t0))
    return _RECORDS[tag]


def _take(w, res):
    """what a call said about one wrapper: the five arrays, best, the record of every entry (fetched at once: the next call drops them)"""
    st, obj, viol, it, route, best = res
    recs = []
    for k in range(len(st)):
        rc, r = w.fixedBatchRecord(k)
        assert rc == (0 if st[k] == 0 else 1), (k, rc, st[k])
        recs.append(r)
    if len(st) == 0:
        assert w.fixedBatchRecord(0) == (-1, None)
    return dict(status=st, objective=obj, violation=viol, iterations=it, route=route, best=best, records=recs)


def _entry_bytes(b, k):
    head = b"".join(np.asarray(b[n][k]).tobytes() for n in ARRAYS)
    return head + (_bytes(b["records"][k], b["objective"][k]) if b["records"][k] is not None else b"")


def _multi(ps, lists):
    ws = [_wrapper(p) for p in ps]
    res = P.solve_fixed_multi(ws, lists)
    return ws, [_take(w, r) for w, r in zip(ws, res)]


def _singles(tags, ps, lists):
    """solveFixedBatch per twin wrapper (kept per tag: the same lists are asked again by other tests); None for an empty list, which the single
    call refuses"""
    out = []
    for tag, p, recs in zip(tags, ps, lists):
        if tag not in _SINGLE:
            w = _wrapper(p)
            _SINGLE[tag] = _take(w, w.solveFixedBatch(recs)) if recs else None
        out.append(_SINGLE[tag])
    return out


def _assert_equal(tag, multi, single, n):
    if single is None:
        assert n == 0 and len(multi["status"]) == 0 and multi["best"] == -1, tag
        return
    assert len(multi["status"]) == n == len(single["status"]), tag
    for a in ARRAYS:
        assert multi[a].tobytes() == single[a].tobytes(), (tag, a, list(multi[a]), list(single[a]))
    assert multi["best"] == single["best"], (tag, multi["best"], single["best"])
    for k in range(n):
        assert _entry_bytes(multi, k) == _entry_bytes(single, k), (tag, k)


def _compare(name, tags, ps, lists):
    ws, multi = _multi(ps, lists)
    single = _singles(tags, ps, lists)
    for h, tag in enumerate(tags):
        _assert_equal(tag, multi[h], single[h], len(lists[h]))
    print("FIXEDMULTI %s entries %s best %s routes %s timing %s" % (name, [len(l) for l in lists], [m["best"] for m in multi],
                                                                    sorted({int(r) for m in multi for r in m["route"]}), ws[0].lastTiming()))
    return ws, multi, single


# ---------------------------------------------------------------------------------------------------------------- the six `mini` handles
def _mini():
    keys = [("mini", seed, 1e-4) for seed in range(6)]
    ps = [_params(k) for k in keys]
    base = [_records_of("mini%d" % s, p) for s, p in enumerate(ps)]
    # alternative 1 of the rear/rear car/car group at step 1 asks car 1, which starts 4 to 12 m ahead, to be behind car 0: infeasible on every seed
    bad = H.infeasible_record(base[1][0], "c2c", (0, 0, 1, 0), 1)
    other = RawResults(1, 2, 16, 1, 0, 0)
    lists = [base[0], [base[1][0], bad, base[1][-1], other, base[1][0]], [], base[3] * 2, base[4] + base[4][:1], base[5] * 3]
    return ["mini%d/%d" % (s, len(l)) for s, l in enumerate(lists)], ps, base, lists


def test_equals_the_single_handle_call():
    """six `mini` instances in one call - a different number of records each, one handle with none, one whose list holds an infeasible and a
    refused record between feasible ones - against solveFixedBatch per twin wrapper: the five arrays, best and every record, as bytes.  The
    same call again gives the same bytes."""
    tags, ps, base, lists = _mini()
    assert len({len(l) for l in lists}) >= 4 and lists[2] == []
    ws, multi, single = _compare("mini", tags, ps, lists)
    assert list(multi[1]["status"]) == [0, 1, 0, 2, 0], list(multi[1]["status"])
    assert multi[1]["route"][3] == -1 and np.isnan(multi[1]["objective"][3]) and multi[1]["best"] in (0, 2)
    for h in (0, 3, 4, 5):
        assert all(s == 0 for s in multi[h]["status"]), (h, list(multi[h]["status"]))
    again = [_take(w, r) for w, r in zip(ws, P.solve_fixed_multi(ws, lists))]
    for h in range(6):
        assert again[h]["best"] == multi[h]["best"]
        assert [_entry_bytes(again[h], k) for k in range(len(lists[h]))] == [_entry_bytes(multi[h], k) for k in range(len(lists[h]))], h
    t = [w.lastTiming() for w in ws]
    assert [x["nodes"] for x in t] == [len(l) - (1 if h == 1 else 0) for h, l in enumerate(lists)]      # (the refused entry is not run)
    assert all(x["ipm_launches"] == 1 and x["solve_s"] == t[0]["solve_s"] and x["ipm_s"] == t[0]["ipm_s"] for x in t)
    assert [x["ipm_iters"] for x in t] == [int(sum(m["iterations"][m["status"] != 2])) for m in multi]


def test_chunk_boundary_inside_a_handle():
    """the six handles with their records repeated to 200 entries each: 1200 nodes in two launch groups, handle 5 on both sides of node 1024.  Every
    copy of a record is byte-equal to the first, and best is the FIRST index of the handle's minimum - the copies tie, across the boundary too"""
    chunk = P.fixed_batch_chunk()
    tags, ps, base, _ = _mini()
    lists = [[b[k % len(b)] for k in range(200)] for b in base]
    assert 5 * 200 < chunk < 6 * 200
    ws, multi = _multi(ps, lists)
    assert all(w.lastTiming()["ipm_launches"] == 2 and w.lastTiming()["nodes"] == 200 for w in ws)
    for h, m in enumerate(multi):
        L = len(base[h])
        first = [_entry_bytes(m, k) for k in range(L)]
        assert all(s == 0 for s in m["status"]), h
        for k in range(200):
            assert _entry_bytes(m, k) == first[k % L], (h, k)
        lowest = min(m["objective"])
        assert m["best"] == min(k for k in range(200) if m["objective"][k] == lowest) < L, (h, m["best"])
    # ... and the first copies are what the single call says about the handle's own records
    for h, (p, b) in enumerate(zip(ps, base)):
        w = _wrapper(p)
        s = _take(w, w.solveFixedBatch(b))
        assert [_entry_bytes(s, k) for k in range(len(b))] == [_entry_bytes(multi[h], k) for k in range(len(b))], h
        assert s["best"] == multi[h]["best"], h


def test_routes_mixed_across_instances():
    """cfg4 seeds 0, 1, 2 (two cars, 20 steps, four obstacles) with their incumbents and pool records - complete records, which on this shape have
    more general rows than either on-chip block holds (route 2) - and, per handle, its incumbent with every leaf disjunction undecided (helpers.relax:
    regions only), which the larger on-chip block solves (route 1): nodes of both launches, of three instances, share one call"""
    ps = [_params(("cfg4", seed, 0.01)) for seed in range(3)]
    lists = []
    for s, p in enumerate(ps):
        recs = _records_of("cfg4s%d" % s, p, cap=8)
        canon = H.canonical_record(recs[0])
        lists.append(recs[:1] + [H.relax(canon, H.leaf_disjunctions(canon))] + recs[1:])
    ws, multi, single = _compare("cfg4", ["cfg4s%d+" % s for s in range(3)], ps, lists)
    routes = {int(r) for m in multi for r in m["route"]}
    assert len(routes) > 1, routes


@pytest.mark.parametrize("cfg", ["mini1", "mini3"])
def test_the_other_kernels(cfg):
    """three one-car instances (mini1: an obstacle, the one-car instantiation of the on-chip kernels) and three three-car instances (mini3: the
    wide memory-backed kernel, two wavefronts per node, route 3), each group in one call"""
    ps = [_params((cfg, seed, 0.01)) for seed in range(3)]
    lists = [_records_of("%ss%d" % (cfg, s), p) for s, p in enumerate(ps)]
    lists[1] = lists[1] * 2
    ws, multi, single = _compare(cfg, ["%ss%d/%d" % (cfg, s, len(l)) for s, l in enumerate(lists)], ps, lists)
    assert all(s == 0 for m in multi for s in m["status"])
    if cfg == "mini3":
        assert {int(r) for m in multi for r in m["route"]} == {3}


def _max_env_edges(p):
    return max(len(np.asarray(e).reshape(-1, 2)) for e in p.MultiEnvironmentConvexPolygon)


def test_different_own_layouts_in_one_call(oracle):
    """Two instances of the same six dimensions whose OWN Layouts differ in EL, the largest number of edges of an environment piece (EL moves SC and
    NSLOT, the slot numbering inside a stage): one call runs both under the common Layout, the single calls each under its own.

    The instances: c2n6e2pent's parameters, and a synthetic.generate instance of its dimensions.  The generator's environment pieces are rectangles,
    and so are both of c2n6e2pent's (its pentagon is the OBSTACLE), so their EL would be 4 and 4; the second instance therefore gets a fifth edge on
    its first piece - the far corner behind the cars cut off - and the test first asserts that the two differ: 4 and 5 edges, and 5 * C * N more
    rows of the raw model (one row per edge and point, rawSizes)."""
    dims = H.shape_dims("c2n6e2pent")
    pa = H.node_instance(oracle, "c2n6e2pent")[0]
    pb = synthetic.generate(dims, 3, gap=1e-4)
    rows4 = _wrapper(pb).rawSizes()["rows"]
    e0 = np.asarray(pb.MultiEnvironmentConvexPolygon[0], float)
    assert e0.shape == (4, 2) and np.array_equal(e0[3], [-10.0, 5.25])
    pb.MultiEnvironmentConvexPolygon[0] = np.array(list(e0[:3]) + [[-8.0, 5.25], [-10.0, 3.25]])   # (counter-clockwise, convex)
    assert H.shape_dims("c2n6e2pent") == (pb.NumCars, pb.NumSteps, pb.nr_regions, pb.nr_environments, pb.nr_obstacles, pb.max_lines_obstacles)
    assert (_max_env_edges(pa), _max_env_edges(pb)) == (4, 5)
    assert _wrapper(pb).rawSizes()["rows"] == rows4 + 5 * pb.NumCars * pb.NumSteps
    lists = [_records_of("c2n6e2pent", pa), _records_of("c2n6e2gen3", pb)]
    for order in ((0, 1), (1, 0)):
        _compare("layouts %s" % (order,), [("c2n6e2pent", "c2n6e2gen3")[k] for k in order], [(pa, pb)[k] for k in order], [lists[k] for k in order])


# ---------------------------------------------------------------------------------------------------------------- pools
def _pool_take(w, res):
    st, obj, viol, it, route = res
    n = w.solutionPoolCount()
    assert len(st) == n
    recs = [w.solutionPoolRecord(k) for k in range(n)]
    assert w.solutionPoolRecord(n)[0] == -1
    return dict(n=n, found=w.solutionPoolFound(), status=st, objective=obj, violation=viol, iterations=it, route=route, rc=[r[0] for r in recs], records=[r[1] for r in recs])


def _pool_entry_bytes(b, k):
    head = b"".join(np.asarray(b[n][k]).tobytes() for n in ARRAYS)
    return head + (_bytes(b["records"][k], b["objective"][k]) if b["records"][k] is not None else b"")


def test_pools_equal_the_single_handle_refinement():
    """the six `mini` instances solved singly with capacity 4 (one with capacity 0), twice - single solves and their pools are reproducible bit for bit.
    One set is refined by solveSolutionPool per wrapper, the twin set by one solve_solution_pools: counts, found objectives, the five arrays and
    every record are equal as bytes; the wrapper without a pool gets count 0 and nothing written"""
    ps = [_params(("mini", seed, 1e-4)) for seed in range(6)]
    sets = []
    for _ in range(2):
        ws = [_wrapper(p, 0 if k == 3 else 4) for k, p in enumerate(ps)]
        assert all(w.callCplex() == P.OptimizationStatus.SUCCESS for w in ws)
        sets.append(ws)
    kept = [[w.solutionPoolCount() for w in ws] for ws in sets]
    assert kept[0] == kept[1] and kept[0][3] == 0 and all(1 <= c <= 4 for k, c in enumerate(kept[0]) if k != 3), kept
    single = [_pool_take(w, w.solveSolutionPool()) for w in sets[0]]
    multi = [_pool_take(w, r) for w, r in zip(sets[1], P.solve_solution_pools(sets[1]))]
    print("POOLMULTI kept %s left %s passes %s / %s" % (kept[0], [m["n"] for m in multi], [w.lastTiming()["ipm_launches"] for w in sets[1]], [w.lastTiming()["ipm_launches"] for w in sets[0]]))
    for h in range(6):
        a, b = single[h], multi[h]
        assert a["n"] == b["n"] and a["rc"] == b["rc"], (h, a["n"], b["n"])
        assert a["found"].tobytes() == b["found"].tobytes(), h
        for n in ARRAYS:
            assert a[n].tobytes() == b[n].tobytes(), (h, n, list(a[n]), list(b[n]))
        assert [_pool_entry_bytes(a, k) for k in range(a["n"])] == [_pool_entry_bytes(b, k) for k in range(b["n"])], h
        ta, tb = sets[0][h].lastTiming(), sets[1][h].lastTiming()
        if h != 3:
            assert (ta["ipm_launches"], ta["nodes"], ta["ipm_iters"], ta["row_iters"]) == (tb["ipm_launches"], tb["nodes"], tb["ipm_iters"], tb["row_iters"]), h
    assert multi[3]["n"] == 0 and len(multi[3]["status"]) == 0
    # the C entry itself: the capacity-0 handle's slots of out[] stay as they were, counts[] and the return value agree
    lib = P.load_library()
    out = (FixedResultC * (6 * 4))()
    for o in out:
        o.status = 9
    counts = (C.c_int * 6)(*([7] * 6))
    left = lib.miqp_solver_pool_solve_multi((C.c_void_p * 6)(*[w._h for w in sets[1]]), 6, out, 4, counts)
    assert list(counts) == [m["n"] for m in multi] and left == sum(counts)
    assert [out[3 * 4 + k].status for k in range(4)] == [9] * 4
    for h in range(6):
        assert [out[h * 4 + k].status for k in range(4)] == [0] * counts[h] + [9] * (4 - counts[h]), h
        assert [np.float64(out[h * 4 + k].objective).tobytes() for k in range(counts[h])] == [np.float64(o).tobytes() for o in multi[h]["objective"]], h


def test_pools_of_a_stream():
    """the `mini` queue drained with two in flight, pool 4 on every handle, and refined in ONE call: per handle entry 0 has the binaries of the
    handle's own result; every entry certifies (status 0, violation < 1e-5, objective within 1e-9 relative: the bounds of the stream test of
    test_solution_pool_gpu.py); refined <= found + 1e-3 |found| (the search finds an entry at node tolerance, loose by at most 0.1 %)"""
    ws = [_wrapper(_params(("mini", seed, 1e-4)), 4) for seed in range(6)]
    sts = P.solve_batch(ws, inflight=2)
    assert all(st == P.OptimizationStatus.SUCCESS for st in sts), sts
    recs = [w.getRawResults() for w in ws]
    kept = [w.solutionPoolCount() for w in ws]
    assert all(1 <= c <= 4 for c in kept), kept
    multi = [_pool_take(w, r) for w, r in zip(ws, P.solve_solution_pools(ws))]
    print("POOLMULTI stream kept %s left %s timing %s" % (kept, [m["n"] for m in multi], ws[0].lastTiming()))
    for h, (w, b) in enumerate(zip(ws, multi)):
        assert 1 <= b["n"] <= kept[h] and b["rc"] == [0] * b["n"], (h, b["rc"])
        for n in BIN:
            assert np.array_equal(getattr(b["records"][0], n), getattr(recs[h], n)), (h, n)
        for j in range(b["n"]):
            assert b["objective"][j] <= b["found"][j] + 1e-3 * abs(b["found"][j]), (h, j, b["objective"][j], b["found"][j])
            cert = w.certify(b["records"][j])
            assert cert.status == 0 and cert.max_violation < 1e-5, (h, j, cert)
            assert abs(cert.objective - b["objective"][j]) <= 1e-9 * max(1.0, abs(b["objective"][j])), (h, j, cert.objective, b["objective"][j])


def test_refusal_on_a_device():
    """a `mini` and a `mini1` handle in one call: -2, and both still hand out the records of their earlier single calls"""
    pa, pb = _params(("mini", 0, 1e-4)), _params(("mini1", 0, 0.01))
    la, lb = _records_of("mini0", pa), _records_of("mini1s0", pb)
    wa, wb = _wrapper(pa), _wrapper(pb)
    before = [_take(w, w.solveFixedBatch(l)) for w, l in ((wa, la), (wb, lb))]
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        P.solve_fixed_multi([wa, wb], [la, lb])
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        P.solve_solution_pools([wa, wb])
    for w, l, b in ((wa, la, before[0]), (wb, lb, before[1])):
        for k in range(len(l)):
            rc, r = w.fixedBatchRecord(k)
            assert rc == 0 and _bytes(r, b["objective"][k]) == _bytes(b["records"][k], b["objective"][k]), k

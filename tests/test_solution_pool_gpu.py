"""The solution pool on the device: what a solve with setSolutionPool(K) keeps, and what solveSolutionPool makes of it.

Instances: two helper shapes the branch and bound solves in milliseconds - c2n6e2pent (two cars, two environment pieces, a pentagon obstacle:
more than one manoeuvre is feasible) and the one-car c1n6r16hex - and seeds 0, 1, 2 of cfg4, the generator's two-car configuration with
obstacles.  Every instance is solved once without and once with a pool, the pool is refined once, and the tests below share those results.
All tests here need a real MI355X: run with  python -m pytest tests/test_solution_pool_gpu.py -m gpu."""
import numpy as np
import pytest

import helpers as H
import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from test_node_qp_gpu import OBJ_RTOL, RAW_TOL, _bytes

pytestmark = pytest.mark.gpu

NAMES = ["c2n6e2pent", "c1n6r16hex", "cfg4s0", "cfg4s1", "cfg4s2"]
CAP = 8
BIN = H.BIN_FIELDS + ["car2car_collision"]
_PARAMS, _SOLVED, _POOLED = {}, {}, {}


def _params(oracle, name):
    """(parameters, oracle handle) - shared and left unchanged"""
    if name not in _PARAMS:
        if name.startswith("cfg4s"):
            p = synthetic.generate("cfg4", int(name[5:]), gap=1e-4)
            _PARAMS[name] = (p, oracle.from_params(p))
        else:
            p, h, dims, rec = H.node_instance(oracle, name)
            _PARAMS[name] = (p, h)
    return _PARAMS[name]


def _solve(oracle, name, cap):
    w = P.CplexWrapper(); w.resetParameters(_params(oracle, name)[0])
    assert w.setSolutionPool(cap) == 0
    st = w.callCplex()
    return dict(w=w, status=st, props=w.getSolutionProperties(), rec=w.getRawResults() if st == P.OptimizationStatus.SUCCESS else None)


def _solved(oracle, name, cap):
    if (name, cap) not in _SOLVED:
        _SOLVED[(name, cap)] = _solve(oracle, name, cap)
    return _SOLVED[(name, cap)]


def _refine(s):
    """count, found objectives, the arrays of solveSolutionPool and every record (fetched at once: the next parameters drop them).  The count and
    the found objectives are read behind the refinement, which merges entries that turn out to be one solution; `kept` is the count before it"""
    w = s["w"]
    kept = w.solutionPoolCount()
    st, obj, viol, it, route = w.solveSolutionPool()
    passes = w.lastTiming()["ipm_launches"]
    n, found = w.solutionPoolCount(), w.solutionPoolFound()
    assert n <= kept and len(obj) == n, (kept, n, len(obj))
    recs = [w.solutionPoolRecord(k) for k in range(n)]
    assert w.solutionPoolRecord(n)[0] == -1
    return dict(n=n, kept=kept, found=found, status=st, objective=obj, violation=viol, iterations=it, route=route, rc=[r[0] for r in recs],
                records=[r[1] for r in recs], passes=passes)


def _pooled(oracle, name):
    if name not in _POOLED:
        s = _solved(oracle, name, CAP)
        assert s["status"] == P.OptimizationStatus.SUCCESS, (name, s["status"])
        _POOLED[name] = _refine(s)
        b = _POOLED[name]
        print("POOL %s kept %d count %d passes %d found %s refined %s" % (name, b["kept"], b["n"], b["passes"], list(b["found"]), list(b["objective"])))
    return _POOLED[name]


def _differ(a, b):
    return any(not np.array_equal(getattr(a, n), getattr(b, n)) for n in BIN)


@pytest.mark.parametrize("name", NAMES)
def test_the_pool_changes_nothing(oracle, name):
    """capacity 0 and capacity 8: the same status and the same bytes of the result record and of the objective - a tree that differs would show here"""
    a, b = _solved(oracle, name, 0), _solved(oracle, name, CAP)
    assert a["status"] == b["status"] == P.OptimizationStatus.SUCCESS
    assert _bytes(a["rec"], a["props"].objective) == _bytes(b["rec"], b["props"].objective), (name, a["props"].objective, b["props"].objective)
    assert a["props"].nodes == b["props"].nodes
    assert a["w"].solutionPoolCount() == 0 and len(a["w"].solutionPoolFound()) == 0


@pytest.mark.parametrize("name", NAMES)
def test_entry_0_is_the_incumbent(oracle, name):
    """the binary arrays of solutionPoolRecord(0) are those of getRawResults(), its refined objective agrees with the solve's within OBJ_RTOL (the
    polish starts warm, the fixed chain cold: no bit equality here)"""
    s, b = _solved(oracle, name, CAP), _pooled(oracle, name)
    assert b["n"] >= 1 and b["rc"][0] == 0 and b["status"][0] == 0
    obj = s["props"].objective
    print("POOL %s entry 0 refined %.12f solve %.12f rel %.2e" % (name, b["objective"][0], obj, abs(b["objective"][0] - obj) / max(1.0, abs(obj))))
    for n in BIN:
        assert np.array_equal(getattr(b["records"][0], n), getattr(s["rec"], n)), (name, n)
    assert abs(b["objective"][0] - obj) <= OBJ_RTOL * max(1.0, abs(obj)), (name, b["objective"][0], obj)


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_is_what_solve_fixed_says(oracle, name):
    """feeding solutionPoolRecord(k) back into solveFixed on the same wrapper: the same objective bytes and the same record bytes as the pool call gave"""
    s, b = _solved(oracle, name, CAP), _pooled(oracle, name)
    for k in range(b["n"]):
        assert b["rc"][k] == 0 and b["status"][k] == 0, (name, k, b["rc"][k], b["status"][k])
        rc, out, obj, it = s["w"].solveFixed(b["records"][k])
        assert rc == 0 and it == b["iterations"][k], (name, k, rc, it, b["iterations"][k])
        assert np.float64(obj).tobytes() == np.float64(b["objective"][k]).tobytes(), (name, k, obj, b["objective"][k])
        assert _bytes(out, obj) == _bytes(b["records"][k], b["objective"][k]), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_is_a_real_solution(oracle, name):
    """per entry: the device certificate is feasible and its objective is the refined one (1e-9 relative, the certificate's tolerance of
    test_certify_gpu.py), the oracle's raw-model violation is below RAW_TOL, and the refined objective is not below the solve's proven bound by
    more than the gap tolerance of the solve"""
    s, b = _solved(oracle, name, CAP), _pooled(oracle, name)
    p, h = _params(oracle, name)
    w = P.CplexWrapper(); w.resetParameters(p)
    for k in range(b["n"]):
        rec, obj = b["records"][k], float(b["objective"][k])
        cert = w.certify(rec)
        v, robj, worst = oracle.raw_eval(h, rec)
        print("POOL %s entry %d refined %.12f certificate %.12f (violation %.2e) oracle violation %.2e bound %.12f" % (name, k, obj, cert.objective, cert.max_violation, v, s["props"].best_bound))
        assert cert.status == 0 and cert.max_violation < 1e-5, (name, k, cert)
        assert abs(cert.objective - obj) <= 1e-9 * max(1.0, abs(obj)), (name, k, cert.objective, obj)
        assert v < RAW_TOL, (name, k, v, worst)
        assert obj >= s["props"].best_bound - p.relative_mip_gap_tolerance * abs(s["props"].objective), (name, k, obj, s["props"].best_bound)


@pytest.mark.parametrize("name", NAMES)
def test_order_and_distinctness(oracle, name):
    """found objectives do not decrease, the records differ pairwise in at least one binary array, the count is at most the capacity (records the
    search kept apart that carry the same binaries are one solution: solveSolutionPool merges them, and the count follows)"""
    b = _pooled(oracle, name)
    assert 1 <= b["n"] <= CAP and len(b["found"]) == b["n"] == len(b["objective"])
    assert all(b["found"][k] <= b["found"][k + 1] for k in range(b["n"] - 1)), list(b["found"])
    for i in range(b["n"]):
        for j in range(i + 1, b["n"]):
            assert _differ(b["records"][i], b["records"][j]), (name, i, j)


@pytest.mark.parametrize("name", ["c2n6e2pent", "cfg4s1"])
def test_capacity_one_keeps_the_incumbent(oracle, name):
    s = _solve(oracle, name, 1)
    assert s["status"] == P.OptimizationStatus.SUCCESS and s["w"].solutionPoolCount() == 1
    b = _refine(s)
    assert b["rc"] == [0]
    for n in BIN:
        assert np.array_equal(getattr(b["records"][0], n), getattr(s["rec"], n)), (name, n)
    assert b["found"][0] == _pooled(oracle, name)["found"][0]


def test_something_is_actually_pooled(oracle):
    """a condition on the inputs, not a measurement of the feature: without an instance that keeps two entries or more, the tests on order,
    distinctness and the entries behind the first would pass on pools of one.  Counts at capacity 8 on an MI355X, as the search kept them ->
    behind the refinement's merge: c2n6e2pent 4 -> 4, c1n6r16hex 4 -> 1 (four records of the incumbent's trajectory), cfg4 seed 0 8 -> 7, seed 1 8 -> 8,
    seed 2 8 -> 8; the six `mini` instances of the stream test at capacity 4: 1, 2, 1, -, 1, 3."""
    counts = {name: _pooled(oracle, name)["n"] for name in NAMES}
    print("POOL counts", counts)
    assert max(counts.values()) >= 2, counts


@pytest.mark.parametrize("name", ["c2n6e2pent", "cfg4s0"])
def test_reproducible(oracle, name):
    """two fresh wrappers on the same instance: the same count, the same found objectives, the same refined bytes"""
    a = _pooled(oracle, name)
    b = _refine(_solve(oracle, name, CAP))
    assert a["n"] == b["n"]
    assert a["found"].tobytes() == b["found"].tobytes()
    for n in ("status", "objective", "violation", "iterations", "route"):
        assert a[n].tobytes() == b[n].tobytes(), (name, n)
    for k in range(a["n"]):
        assert _bytes(a["records"][k], a["objective"][k]) == _bytes(b["records"][k], b["objective"][k]), (name, k)


def test_a_refused_capacity_leaves_the_previous_one_in_force(oracle):
    """capacity 4 accepted, then 99 and -1 refused: the next solve keeps at most 4 entries and at least the incumbent (cfg4 seed 1 keeps 8 at capacity 8,
    so a setting of 0 or of the maximum would show)"""
    w = P.CplexWrapper(); w.resetParameters(_params(oracle, "cfg4s1")[0])
    assert P.pool_max() < 99
    assert w.setSolutionPool(4) == 0 and w.setSolutionPool(99) < 0 and w.setSolutionPool(-1) < 0
    assert w.callCplex() == P.OptimizationStatus.SUCCESS
    n = w.solutionPoolCount()
    print("POOL cfg4s1 capacity 4 (99 and -1 refused) count", n)
    assert 1 <= n <= 4, n


_MINI = []


def _mini():
    if not _MINI:
        _MINI.extend(synthetic.generate("mini", seed, gap=1e-4) for seed in range(6))
    return _MINI


def test_stream_one_in_flight(oracle):
    """six instances drained with ONE in flight, pool 4 on every handle: every instance's end is a round without a batch, hence without a capture,
    and the next instance's first candidates come in the round after it.  Each handle's entry 0 has its own result's binaries, every entry
    certifies, the found objectives do not decrease, and every found objective is a primal value of its entry: the refined objective is the
    minimum of a QP whose feasible set holds the optimum of the entry's record (the refinement re-labels from that optimum), and the search
    found the entry at node tolerance, loose by at most 0.1 % of the objective (kernels.hip, QP_TOL) - so refined <= found + 1e-3 |found|.  A found
    objective taken from another node's relaxation lies below that."""
    ws = []
    for p in _mini():
        w = P.CplexWrapper(); w.resetParameters(p)
        assert w.setSolutionPool(4) == 0
        ws.append(w)
    sts = P.solve_batch(ws, inflight=1)
    assert all(st == P.OptimizationStatus.SUCCESS for st in sts), sts
    recs = [w.getRawResults() for w in ws]
    counts = [w.solutionPoolCount() for w in ws]
    print("POOL stream, one in flight, counts", counts)
    assert all(1 <= c <= 4 for c in counts), counts
    for k, w in enumerate(ws):
        b = _refine(dict(w=w))
        print("POOL stream, one in flight, %d found %s refined %s" % (k, list(b["found"]), list(b["objective"])))
        assert b["n"] >= 1 and b["rc"] == [0] * b["n"], (k, b["rc"])
        for n in BIN:
            assert np.array_equal(getattr(b["records"][0], n), getattr(recs[k], n)), (k, n)
        assert all(b["found"][j] <= b["found"][j + 1] for j in range(b["n"] - 1)), (k, list(b["found"]))
        for j in range(b["n"]):
            assert b["objective"][j] <= b["found"][j] + 1e-3 * abs(b["found"][j]), (k, j, b["objective"][j], b["found"][j])
            cert = w.certify(b["records"][j])
            assert cert.status == 0 and cert.max_violation < 1e-5, (k, j, cert)
            assert abs(cert.objective - b["objective"][j]) <= 1e-9 * max(1.0, abs(b["objective"][j])), (k, j, cert.objective, b["objective"][j])


def test_stream(oracle):
    """six instances drained with two in flight, pool 4 on every handle but one: each handle's entry 0 has its own result's binaries, every entry
    certifies, and the handle with capacity 0 in the same call reports a count of 0"""
    ps = _mini()
    ws = []
    for k, p in enumerate(ps):
        w = P.CplexWrapper(); w.resetParameters(p)
        assert w.setSolutionPool(0 if k == 3 else 4) == 0
        ws.append(w)
    sts = P.solve_batch(ws, inflight=2)
    assert all(st == P.OptimizationStatus.SUCCESS for st in sts), sts
    recs = [w.getRawResults() for w in ws]
    counts = [w.solutionPoolCount() for w in ws]
    print("POOL stream counts", counts)
    assert counts[3] == 0 and all(1 <= c <= 4 for k, c in enumerate(counts) if k != 3), counts
    for k, w in enumerate(ws):
        if k == 3:
            continue
        b = _refine(dict(w=w))
        assert b["rc"] == [0] * b["n"], (k, b["rc"])
        for n in BIN:
            assert np.array_equal(getattr(b["records"][0], n), getattr(recs[k], n)), (k, n)
        for j in range(b["n"]):
            cert = w.certify(b["records"][j])
            assert cert.status == 0 and cert.max_violation < 1e-5, (k, j, cert)
            assert abs(cert.objective - b["objective"][j]) <= 1e-9 * max(1.0, abs(b["objective"][j])), (k, j, cert.objective, b["objective"][j])

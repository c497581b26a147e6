"""Starts from the carried pool on the device (setSolutionPoolStarts, solutionPoolStartsLast): the solve behind a carry into an EMPTY pool
takes the carried records as MIP-start roots of its first round.

Fixtures and set-up are those of test_pool_carry_gpu.py: c2n6e2pent and wrap (sources at capacity 8), cfg4 seeds 12 and 5 (sources at capacity 16),
every source solved under filter 12 and explored (settled), the destination advanced one step along the source's solution.  Every destination here
has capacity 16 and filter 12 and is solved at gap 1e-7 (gap_override), its fresh twin - the same wrapper without a carry and with the switch off -
included.  The carry into the empty destination admits m >= 1 records on all four, and every test asserts it for its fixture (cfg4 seed 12
with DESIGN 6l's two carried classes: m >= 2); what each admits is printed.
For the record (one MI355X; test_it_does_something prints it): the carries admit m = 1, 1, 3 and 9 records, every start has a place, the pools
behind the solve hold 2, 1, 3 and 10 entries (fresh: 1, 1, 1, 7) and the solves relax 11, 3, 11 and 4202 nodes (fresh: 26, 2, 16, 25700).
All tests here need a real MI355X: run with  python -m pytest tests/test_pool_starts_gpu.py -m gpu -s."""
import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import SolutionPropertiesC
from test_pool_carry_gpu import _dst_params, _source
from test_pool_explore_gpu import _same_solve
from test_pool_filter_gpu import FILTER, _as_found

pytestmark = pytest.mark.gpu

CASES = [("c2n6e2pent", 8), ("wrap", 8), ("cfg4s12", 16), ("cfg4s5", 16)]
IDS = ["%s-%d" % c for c in CASES]
GAP = 1e-7
CAP = 16
TOP = 16   # pool_max(): the most starts
_FRESH, _STARTED = {}, {}


def _wrapper(name, cap, starts):
    """a destination with its instance loaded, capacity and filter set and no solve.  The switch is set BEFORE the parameters are loaded: that it
    holds in the solve is the library's "the setting survives miqp_solver_set_params\""""
    w = P.CplexWrapper(gap_override=GAP)
    assert w.setSolutionPoolStarts(starts) == 0
    w.resetParameters(_dst_params(name, cap, 1, "plain"))
    assert w.setSolutionPool(CAP) == 0 and w.setSolutionPoolFilter(FILTER) == 0
    assert w._loaded() and w.solutionPoolStartsLast() == [] and w.solutionPoolStarts() == starts
    return w


def _pool(w):
    n = w.solutionPoolCount()
    return dict(n=n, found=w.solutionPoolFound(), dec=[w.solutionPoolFoundDecisions(k) for k in range(n)])


def _fresh(name, cap):
    """the destination solved on a fresh wrapper without starts (shared and left unchanged)"""
    if (name, cap) not in _FRESH:
        w = _wrapper(name, cap, 0)
        s = _as_found(w, w.callCplex())
        assert s["status"] == P.OptimizationStatus.SUCCESS and w.solutionPoolStartsLast() == [], (name, s["status"])
        _FRESH[(name, cap)] = s
    return _FRESH[(name, cap)]


def _carry_then_solve(name, cap, starts=TOP, between=None):
    """a fresh destination, the carry into its empty pool, `between` (a callable on the wrapper, or None), the solve"""
    w = _wrapper(name, cap, starts)
    m, out = w.carrySolutionPool(_source(name, cap)["w"], 1, -1.0)
    assert m >= 0 and w.solutionPoolCount() == m, (name, m)
    before = _pool(w)
    if between is not None:
        between(w)
    s = _as_found(w, w.callCplex())
    s.update(m=m, before=before, places=w.solutionPoolStartsLast())
    return s


def _started(name, cap):
    """case 1, shared and left unchanged"""
    if (name, cap) not in _STARTED:
        _STARTED[(name, cap)] = _carry_then_solve(name, cap)
    return _STARTED[(name, cap)]


def _takes_part(name, cap):
    """case 1 of a fixture.  The carry into the empty destination admits at least one record on every one of the four (recorded: 1, 1, 3, 9):
    a fixture that stopped admitting would have nothing to start from, and its tests fail here instead of passing empty"""
    s = _started(name, cap)
    assert s["m"] >= 1, (name, "the carry into the empty destination admits nothing")
    return s


def _refuse_out_of_range(w):
    assert [w.setSolutionPoolStarts(v) for v in (-1, TOP + 1)] == [-1, -1]


def _props(s):
    return {n: getattr(s["props"], n) for n, _ in SolutionPropertiesC._fields_ if n != "time"}


def _same_as_fresh(name, cap, s, what):
    f = _fresh(name, cap)
    _same_solve(f, s, (name, what))
    a, b = _props(f), _props(s)
    assert {k: np.float64(v).tobytes() for k, v in a.items()} == {k: np.float64(v).tobytes() for k, v in b.items()}, (name, what, a, b)
    assert s["places"] == [], (name, what, s["places"])


def test_it_does_something():
    """conditions on the inputs: the carry into the empty pool admits on every fixture (recorded: 1, 1, 3 and 9 records).  What every fixture
    gives is printed for the record"""
    m = {}
    for name, cap in CASES:
        s, f = _started(name, cap), _fresh(name, cap)
        m[name] = s["m"]
        print("STARTS %s: carried %d, T %d places %s, entries %d (fresh %d), objective %.9g (fresh %.9g), nodes %d (fresh %d), found before %s after %s"
              % (name, s["m"], len(s["places"]), s["places"], s["n"], f["n"], s["props"].objective, f["props"].objective, s["props"].nodes, f["props"].nodes,
                 list(s["before"]["found"]), list(s["found"])))
    assert all(v >= 1 for v in m.values()) and m["cfg4s12"] >= 2, m


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_answer(name, cap):
    """case 1: SUCCESS, a certified record, the fresh solve's objective to the parity suite's 1e-6, and T = min(16, m)"""
    s, f = _takes_part(name, cap), _fresh(name, cap)
    assert s["status"] == P.OptimizationStatus.SUCCESS, (name, s["status"])
    cert = s["w"].certify(s["rec"])
    assert cert.status == 0 and cert.max_violation < 1e-5, (name, cert)
    assert abs(s["props"].objective - f["props"].objective) <= 1e-6 * max(1.0, abs(f["props"].objective)), (name, s["props"].objective, f["props"].objective)
    assert len(s["places"]) == min(TOP, s["m"]), (name, s["places"], s["m"])


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_fallback_survives_the_solve(name, cap):
    """case 2: below capacity every start stands in the pool behind the solve; at capacity a start without a place is not better than the last entry"""
    s = _takes_part(name, cap)
    assert all(-1 <= p < s["n"] for p in s["places"]), (name, s["places"], s["n"])
    if s["n"] < CAP:
        assert all(p >= 0 for p in s["places"]), (name, s["places"], s["n"])
    else:
        for k, p in enumerate(s["places"]):
            assert p >= 0 or s["before"]["found"][k] >= s["found"][-1], (name, k, s["before"]["found"][k], s["found"][-1])
    # under the filter a start's place is the entry of its signature
    Cn, N, O = s["dims"]
    sig = lambda d: P.pool_signature(Cn, N, O, FILTER, d).tobytes()   # noqa: E731
    for k, p in enumerate(s["places"]):
        if p >= 0:
            assert sig(s["before"]["dec"][k]) == sig(s["dec"][p]), (name, k, p)
        else:
            assert sig(s["before"]["dec"][k]) not in [sig(d) for d in s["dec"]], (name, k)


def test_cfg4_seed_12_keeps_more_classes_than_the_solve_alone():
    """the fixture of DESIGN 6l - one class from the solve alone, two carried: behind a solve with starts the pool is below capacity and holds them all"""
    s, f = _takes_part("cfg4s12", 16), _fresh("cfg4s12", 16)
    assert s["n"] < CAP and all(p >= 0 for p in s["places"]) and len(set(s["places"])) == len(s["places"]), (s["n"], s["places"])
    print("STARTS cfg4s12: %d entries behind the solve with starts, %d behind the fresh solve" % (s["n"], f["n"]))


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_a_start_cap(name, cap):
    """case 3: max_starts = 1 takes entry 0 of the carried pool; a refused value in between leaves the setting alone"""
    _takes_part(name, cap)
    s = _carry_then_solve(name, cap, 1, _refuse_out_of_range)
    assert s["status"] == P.OptimizationStatus.SUCCESS and len(s["places"]) == 1, (name, s["places"])
    Cn, N, O = s["dims"]
    p = s["places"][0]
    if p >= 0:
        assert P.pool_signature(Cn, N, O, FILTER, s["before"]["dec"][0]).tobytes() == P.pool_signature(Cn, N, O, FILTER, s["dec"][p]).tobytes(), (name, p)
    else:
        assert s["n"] == CAP and s["before"]["found"][0] >= s["found"][-1], (name, s["n"])


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_off_means_off(name, cap):
    """case 4: the switch off behind the same carry, the switch on without a carry, and the switch on with the carried pool dropped by new
    parameters are each the fresh solve, byte for byte"""
    _takes_part(name, cap)
    _same_as_fresh(name, cap, _carry_then_solve(name, cap, 0), "max_starts 0 behind the carry")
    w = _wrapper(name, cap, TOP)
    s = _as_found(w, w.callCplex()); s["places"] = w.solutionPoolStartsLast()
    _same_as_fresh(name, cap, s, "max_starts 16 without a carry")
    _same_as_fresh(name, cap, _carry_then_solve(name, cap, TOP, lambda w: w.resetParameters(_dst_params(name, cap, 1, "plain"))), "the carried pool dropped by resetParameters")


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_reproducible(name, cap):
    """case 5: two fresh runs give the same record, pool and places, byte for byte"""
    a = _takes_part(name, cap)
    b = _carry_then_solve(name, cap)
    _same_solve(a, b, (name, "a second run"))
    assert a["places"] == b["places"] and a["m"] == b["m"], (name, a["places"], b["places"])


def test_a_batch_with_and_without_starts():
    """case 6: one solve_batch over four handles of cfg4 seed 12's destination - two carried into with the switch on, one with the switch on and no
    carry, one carried into with the switch off; then the same four again, none with a carried pool (five root records per instance again)"""
    name, cap = "cfg4s12", 16
    _takes_part(name, cap)
    f = _fresh(name, cap)
    src = _source(name, cap)["w"]
    ws = [_wrapper(name, cap, TOP), _wrapper(name, cap, TOP), _wrapper(name, cap, TOP), _wrapper(name, cap, 0)]
    m = [ws[k].carrySolutionPool(src, 1, -1.0)[0] for k in (0, 1, 3)]
    assert m[0] == m[1] == m[2] == _started(name, cap)["m"]
    want = [min(TOP, m[0]), min(TOP, m[1]), 0, 0]
    for again in (False, True):
        st = P.solve_batch(ws)
        assert st == [P.OptimizationStatus.SUCCESS] * 4, (again, st)
        for k, w in enumerate(ws):
            o = w.getSolutionProperties().objective
            assert abs(o - f["props"].objective) <= 1e-6 * max(1.0, abs(f["props"].objective)), (again, k, o, f["props"].objective)
            assert len(w.solutionPoolStartsLast()) == (0 if again else want[k]), (again, k, w.solutionPoolStartsLast())
            assert w.certify(w.getRawResults()).status == 0, (again, k)


def test_pool_calls_behind_such_a_solve_and_the_next_cycle():
    """case 7: solveSolutionPool behind a solve with starts and its records certify; the pool carries on into the next cycle's destination, whose
    solve starts from it in turn"""
    name, cap = "cfg4s12", 16
    _takes_part(name, cap)
    s = _carry_then_solve(name, cap)
    w = s["w"]
    nxt = P.CplexWrapper(gap_override=GAP)
    assert nxt.setSolutionPoolStarts(TOP) == 0
    nxt.resetParameters(synthetic.advance(_dst_params(name, cap, 1, "plain"), s["rec"], 1))
    assert nxt.setSolutionPool(CAP) == 0 and nxt.setSolutionPoolFilter(FILTER) == 0 and nxt._loaded()
    m2, out = nxt.carrySolutionPool(w, 1, -1.0)
    assert m2 >= 0 and len(out) == s["n"], (m2, len(out), s["n"])
    st2 = nxt.callCplex()
    assert st2 == P.OptimizationStatus.SUCCESS and len(nxt.solutionPoolStartsLast()) == min(TOP, m2), (st2, m2, nxt.solutionPoolStartsLast())
    assert nxt.certify(nxt.getRawResults()).status == 0
    print("STARTS chain: cycle 1 keeps %d entries, cycle 2 is carried %d, takes %d starts, keeps %d entries" % (s["n"], m2, len(nxt.solutionPoolStartsLast()), nxt.solutionPoolCount()))
    st, obj, viol, it, route = w.solveSolutionPool()
    assert len(obj) == w.solutionPoolCount() >= 1
    for k in range(len(obj)):
        rc, rec = w.solutionPoolRecord(k)
        assert (rc == 0) == (st[k] == 0), (k, rc, st[k])
        if rc == 0:
            cert = w.certify(rec)
            assert cert.status == 0 and cert.max_violation < 1e-5, (k, cert)
    assert st[0] == 0

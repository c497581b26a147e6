"""The free places of a filtered solution pool filled with neighbouring manoeuvre classes on the device (exploreSolutionPool).

Instances, under filter 12: c2n6e2pent at capacity 8 (N = 6, the smallest shape), wrap at capacity 8 ((2, 6, 32, 2, 6) seed 0: 76 sites and 12 groups,
the loop over the units wraps past 64 lanes), cfg4 seeds 7 and 12 at capacity 16 (their pools hold ONE entry: the case the call exists for), cfg4
seed 1 at capacity 8 and cfg4 seed 9 at capacity 16 (a full pool: the call returns 0 and touches nothing).  Every solve and every call runs once on a
fresh wrapper and is kept for the tests that share it.

The reference of the call is its HOST REPLAY (_replay): pool_jumps on the bytes of each expanded entry, all neighbours of a pass through one
solveDecisions call, the feasible ones visited in ascending (objective, neighbour number), classes told apart with pool_signature, the cost cap
restated, the stopping rules - host code that uses neither of the two new kernels; the chain behind solveDecisions is the fixed batch's, which its own
suite pins.  Both sides are bit for bit.
For the record (one MI355X, no cap, up to 4 passes): the replay admits 6, 7, 15, 15, 6 and 0 entries on the six instances, every one in pass 1.  Most
of them have the incumbent's objective to 13 digits - the same trajectory under labels of another signature that hold as well - and
solveSolutionPool merges them again (16 -> 1 entries left on seed 7, 16 -> 3 on seed 12, whose other two are new manoeuvres at 309.2 and 812.3
against the incumbent's 272.9): DESIGN.md 6h says what follows from that.
All tests here need a real MI355X: run with  python -m pytest tests/test_pool_explore_gpu.py -m gpu -s."""
import ctypes as C

import numpy as np
import pytest

import planner_miqp_amd as P
from test_node_qp_gpu import _bytes
from test_pool_filter_gpu import FILTER, _as_found, _params

pytestmark = pytest.mark.gpu

CASES = [("c2n6e2pent", 8), ("wrap", 8), ("cfg4s7", 16), ("cfg4s12", 16), ("cfg4s1", 8), ("cfg4s9", 16)]
IDS = ["%s-%d" % c for c in CASES]
FULL = ("cfg4s9", 16)
PASSES = [1, 4]
MAX_REL = [-1.0, 0.5]
_SOLVED, _EXPLORED, _REPLAY = {}, {}, {}


def _fresh(name, cap):
    w = P.CplexWrapper(); w.resetParameters(_params(name))
    assert w.setSolutionPool(cap) == 0 and w.setSolutionPoolFilter(FILTER) == 0
    s = _as_found(w, w.callCplex())
    assert s["status"] == P.OptimizationStatus.SUCCESS and s["n"] >= 1, (name, cap, s["status"], s["n"])
    d = (C.c_int * 6)()
    assert w._L.miqp_solver_get_dims(w._h, d) == 0
    s["lines"] = d[5]
    return s


def _solved(name, cap):
    """a solve whose pool nothing touches"""
    if (name, cap) not in _SOLVED:
        _SOLVED[(name, cap)] = _fresh(name, cap)
    return _SOLVED[(name, cap)]


def _timing(w):
    t = (C.c_double * 6)()
    assert w._L.miqp_solver_last_timing(w._h, t) == 0
    return list(t)


def _explored(name, cap, passes, max_rel):
    """a fresh solve and exploreSolutionPool(passes, max_rel) behind it: the pool as found, the call's answer and timing, the pool it leaves"""
    key = (name, cap, passes, max_rel)
    if key not in _EXPLORED:
        s = _fresh(name, cap)
        w = s["w"]
        rc, added = w.exploreSolutionPool(passes, max_rel)
        t = _timing(w)
        n = w.solutionPoolCount()
        _EXPLORED[key] = dict(w=w, solved=s, rc=rc, added=added, timing=t, err=w.lastError(), n=n, found=w.solutionPoolFound(),
                              dec=[w.solutionPoolFoundDecisions(k) for k in range(n)])
        print("EXPLORE %s capacity %d passes %d max_rel %g: %d entries, rc %d, passes run %d, neighbours %d, iterations %d, still adding %d, device %.1f ms of %.1f ms"
              % (name, cap, passes, max_rel, s["n"], rc, t[2], t[3], t[4], t[5], 1e3 * t[1], 1e3 * t[0]))
        for a in added:
            print("EXPLORE %s capacity %d: + pass %d parent %d jump (%d, %d, %d, %d) objective %.6f (entry 0: %.6f)"
                  % (name, cap, a["pass"], a["parent"], a["first"], a["stride"], a["count"], a["value"], a["objective"], s["found"][0]))
    return _EXPLORED[key]


def _within(obj0, obj, max_rel):
    """the cost cap: objective - obj0 <= max_rel |obj0|, every operation rounded on its own"""
    return max_rel < 0 or np.float64(obj) - np.float64(obj0) <= np.float64(max_rel) * abs(np.float64(obj0))


def _replay(name, cap, max_rel):
    """the call as a host loop over pool_jumps and solveDecisions, up to 4 passes: the state behind every pass that ran (0: the pool as found)"""
    if (name, cap, max_rel) in _REPLAY:
        return _REPLAY[(name, cap, max_rel)]
    s = _solved(name, cap)
    Cn, N, O = s["dims"]
    w = P.CplexWrapper(); w.resetParameters(_params(name))
    dec, found = [d.copy() for d in s["dec"]], [float(x) for x in s["found"]]
    sigs = [P.pool_signature(Cn, N, O, FILTER, d).tobytes() for d in dec]
    added, expand = [], list(range(len(dec)))
    neighbours = iterations = 0
    states = {0: dict(added=[], dec=list(dec), found=list(found), passes=0, neighbours=0, iterations=0, last=0)}
    for p in range(1, 5):
        if len(dec) >= cap:
            break
        lists = [P.pool_jumps(Cn, N, O, s["lines"], FILTER, dec[k]) for k in expand]
        total = sum(len(m) for m in lists)
        if total == 0:
            break
        recs = np.empty((total, dec[0].size), dtype=np.int8)
        origin = []
        for k, mv in zip(expand, lists):
            for first, stride, count, value in mv:
                recs[len(origin)] = dec[k]
                recs[len(origin), first:first + count * stride:stride] = value
                origin.append((k, int(first), int(stride), int(count), int(value)))
        rc, st, obj, viol, it, route, best = w.solveDecisions(recs)
        assert rc == 0 and not (st == 2).any(), (name, p)   # (every jump is a record of valid alternatives)
        neighbours += total; iterations += int(it.sum())
        new = []
        for g in sorted((g for g in range(total) if st[g] == 0), key=lambda g: (obj[g], g)):
            if len(dec) >= cap:
                break
            sg = P.pool_signature(Cn, N, O, FILTER, recs[g]).tobytes()
            if not _within(found[0], obj[g], max_rel) or sg in sigs:
                continue
            k, first, stride, count, value = origin[g]
            new.append(len(dec))
            added.append({"parent": k, "pass": p, "first": first, "stride": stride, "count": count, "value": value, "iterations": int(it[g]), "objective": float(obj[g])})
            dec.append(recs[g].copy()); found.append(float(obj[g])); sigs.append(sg)
        print("REPLAY %s capacity %d max_rel %g pass %d: %d expanded, %d neighbours, %d feasible, %d admitted"
              % (name, cap, max_rel, p, len(expand), total, int((st == 0).sum()), len(new)))
        states[p] = dict(added=list(added), dec=list(dec), found=list(found), passes=p, neighbours=neighbours, iterations=iterations, last=len(new))
        if not new:
            break
        expand = new
    _REPLAY[(name, cap, max_rel)] = states
    return states


def _same_solve(a, b, what):
    assert a["status"] == b["status"] == P.OptimizationStatus.SUCCESS, what
    assert _bytes(a["rec"], a["props"].objective) == _bytes(b["rec"], b["props"].objective), what
    assert a["props"].nodes == b["props"].nodes and a["n"] == b["n"], what
    assert a["found"].tobytes() == b["found"].tobytes(), what
    for k in range(a["n"]):
        assert a["dec"][k].tobytes() == b["dec"][k].tobytes(), (what, k)


def test_it_does_something():
    """a condition on the inputs, checked on the REPLAY: over the instances at least one entry is admitted without a cap.  What each admitted is
    printed for the record"""
    admitted = {}
    for name, cap in CASES:
        states = _replay(name, cap, -1.0)
        e = states[max(states)]
        admitted[(name, cap)] = [(a["pass"], a["parent"], a["objective"]) for a in e["added"]]
        print("REPLAY %s capacity %d: %d entries found, admitted %s" % (name, cap, _solved(name, cap)["n"], admitted[(name, cap)]))
    assert any(admitted.values()), admitted
    assert _solved(*FULL)["n"] == FULL[1] and not admitted[FULL]   # (the full pool of the suite is full)


@pytest.mark.parametrize("max_rel", MAX_REL)
@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_explore_is_its_host_replay(name, cap, passes, max_rel):
    states = _replay(name, cap, max_rel)
    c = _explored(name, cap, passes, max_rel)
    s = c["solved"]
    e = states[min(passes, max(states))]
    assert c["rc"] == len(e["added"]) == len(c["added"]) and c["n"] == len(e["dec"]) == s["n"] + c["rc"]
    for a, b in zip(c["added"], e["added"]):
        assert {k: v for k, v in a.items() if k != "objective"} == {k: v for k, v in b.items() if k != "objective"}, (a, b)
        assert np.float64(a["objective"]).tobytes() == np.float64(b["objective"]).tobytes(), (a, b)
    assert c["found"].tobytes() == np.array(e["found"], dtype=np.float64).tobytes(), (list(c["found"]), e["found"])
    for k in range(c["n"]):
        assert c["dec"][k].tobytes() == e["dec"][k].tobytes(), (name, cap, passes, k)
    for k in range(s["n"]):   # old entries are the same bytes before and after
        assert c["dec"][k].tobytes() == s["dec"][k].tobytes() and np.float64(c["found"][k]).tobytes() == np.float64(s["found"][k]).tobytes(), (name, k)
    assert ((name, cap) == FULL) == (s["n"] >= cap), (name, cap, s["n"])
    if (name, cap) == FULL:
        assert c["rc"] == 0 and c["err"] == ""
        return   # (no device work: the timing is still the solve's)
    t = c["timing"]
    still = 1 if e["passes"] == passes and e["last"] > 0 else 0
    assert (t[2], t[3], t[4], t[5]) == (e["passes"], e["neighbours"], e["iterations"], still), (t, e["passes"], e["neighbours"], e["iterations"], still)
    assert ("still added" in c["err"]) == bool(still and c["n"] < cap)


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_properties(name, cap):
    """the signatures of the pool are pairwise distinct, every added objective respects the cap, every added entry is what solveDecisions answers
    for its bytes, and its bytes are its parent's behind its jump"""
    Cn, N, O = _solved(name, cap)["dims"]
    w2 = P.CplexWrapper(); w2.resetParameters(_params(name))
    for max_rel in MAX_REL:
        c = _explored(name, cap, 4, max_rel)
        s = c["solved"]
        sigs = [P.pool_signature(Cn, N, O, FILTER, d).tobytes() for d in c["dec"]]
        assert len(set(sigs)) == len(sigs) == c["n"] <= cap, (name, max_rel)
        if not c["added"]:
            continue
        new = np.stack(c["dec"][s["n"]:])
        rc, st, obj, viol, it, route, best = w2.solveDecisions(new)
        assert rc == 0 and (st == 0).all()
        for j, a in enumerate(c["added"]):
            assert _within(s["found"][0], a["objective"], max_rel), (name, max_rel, a)
            assert np.float64(a["objective"]).tobytes() == np.float64(obj[j]).tobytes() == np.float64(c["found"][s["n"] + j]).tobytes(), (name, j)
            assert a["iterations"] == it[j] and 1 <= a["pass"] <= 4 and 0 <= a["parent"] < s["n"] + j
            want = c["dec"][a["parent"]].copy()
            want[a["first"]:a["first"] + a["count"] * a["stride"]:a["stride"]] = a["value"]
            assert want.tobytes() == new[j].tobytes(), (name, j)
            if a["pass"] > 1:
                assert c["added"][a["parent"] - s["n"]]["pass"] == a["pass"] - 1


@pytest.mark.parametrize("name,cap", [CASES[0], CASES[1], CASES[2], CASES[4]], ids=[IDS[0], IDS[1], IDS[2], IDS[4]])
def test_reproducible(name, cap):
    a = _explored(name, cap, 4, -1.0)
    _EXPLORED.pop((name, cap, 4, -1.0))
    b = _explored(name, cap, 4, -1.0)
    assert a["rc"] == b["rc"] and a["n"] == b["n"] and a["timing"][2:] == b["timing"][2:] and a["found"].tobytes() == b["found"].tobytes()
    assert [sorted(x.items()) for x in a["added"]] == [sorted(x.items()) for x in b["added"]]
    for k in range(a["n"]):
        assert a["dec"][k].tobytes() == b["dec"][k].tobytes(), (name, k)


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_solve_is_untouched(name, cap):
    """the exploring wrapper's own solve was the solve of a wrapper nothing touched, and a solve BEHIND an explore on the same wrapper equals a fresh one"""
    a = _solved(name, cap)
    c = _explored(name, cap, 1, -1.0)
    _same_solve(a, c["solved"], (name, cap, "the exploring wrapper's own solve"))
    _same_solve(a, _as_found(a["w"], a["status"]), (name, cap, "the untouched wrapper behind the other's explore"))
    w = c["w"]
    _same_solve(a, _as_found(w, w.callCplex()), (name, cap, "a solve behind an explore"))
    _EXPLORED.pop((name, cap, 1, -1.0))   # (its pool is the new solve's now)


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_climb_and_refinement_behind_the_explore(name, cap):
    """improveSolutionPool and solveSolutionPool work on the larger pool as on any other: the climb leaves every entry in its class and no worse, the
    refinement hands out records that certify"""
    c = _explored(name, cap, 4, -1.0)
    _EXPLORED.pop((name, cap, 4, -1.0))   # (its pool is the climbed and refined one from here on)
    w, n = c["w"], c["n"]
    Cn, N, O = c["solved"]["dims"]
    rc, before, after, moves, status = w.improveSolutionPool(8)
    assert rc >= 0 and len(before) == n == w.solutionPoolCount(), (name, rc)
    for k in range(n):
        assert P.pool_signature(Cn, N, O, FILTER, w.solutionPoolFoundDecisions(k)).tobytes() == P.pool_signature(Cn, N, O, FILTER, c["dec"][k]).tobytes(), (name, k)
        assert after[k] <= before[k]
        if k >= c["solved"]["n"]:   # an added entry was found at the tight tolerance: the climb's pass 0 answers with the same bits
            assert status[k] == 0 and np.float64(before[k]).tobytes() == np.float64(c["found"][k]).tobytes(), (name, k)
    st, obj, viol, it, route = w.solveSolutionPool()
    assert 1 <= len(obj) == w.solutionPoolCount() <= n
    certified = 0
    for k in range(len(obj)):
        rc, rec = w.solutionPoolRecord(k)
        assert (rc == 0) == (st[k] == 0), (name, k, rc, st[k])
        if rc != 0:
            continue
        cert = w.certify(rec)
        assert cert.status == 0 and cert.max_violation < 1e-5, (name, k, cert)
        certified += 1
    assert certified >= 1
    print("BEHIND %s capacity %d: %d entries, %d climbed, %d left by the refinement, %d certified" % (name, cap, n, int((moves > 0).sum()), len(obj), certified))

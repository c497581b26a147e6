"""The climb of a filtered solution pool inside its manoeuvre classes on the device (improveSolutionPool, solveDecisions).

Instances: the pool-filter suite's - c2n6e2pent (N = 6, the smallest shape), wrap ((2, 6, 32, 2, 6) seed 0: 76 sites, the loop over the sites wraps past
64 lanes) and cfg4 seeds 1, 4 and 9 at gap 1e-4 (fix record of 80 16-byte chunks, N = 20) - under filter 12 at capacity 8, seed 9 also at capacity 16
(the full filtered pool of DESIGN.md 6e).  Every solve and every climb runs once on a fresh wrapper and is kept for the tests that share it.

The reference of the climb is its HOST REPLAY (_replay): pool_moves on each entry's current bytes, all neighbours through one solveDecisions call,
argmin over status 0 with ties to the lower move number, the acceptance rule, repeat - host code that uses none of the three new kernels of the climb; the
chain behind solveDecisions is the fixed batch's, which its own suite pins.  Both sides are bit for bit.
All tests here need a real MI355X: run with  python -m pytest tests/test_pool_improve_gpu.py -m gpu -s."""
import numpy as np
import pytest

import planner_miqp_amd as P
from test_node_qp_gpu import OBJ_RTOL, _bytes
from planner_miqp_amd import synthetic
from test_pool_filter_gpu import FILTER, _as_found
from test_pool_filter_gpu import _params as _filter_params

pytestmark = pytest.mark.gpu

# a 76-site shape again, with a horizon, a seed and a filter under which a kept entry has moves on sites below 64 AND on sites 64 .. 75: 8 moves, 4
# of them past lane 63 (seed 0 of `wrap` keeps one leaf without a change point; of (2, 6, 32, 2, 6) no seed 0 .. 15 has an entry whose moves cross
# the block under filter 1, 2, 3, 8 or 12, so the horizon is 8 here: seeds 3, 10 and 11 cross).  None of its 8 neighbours improves the entry
WRAP2_CFG, WRAP2_SEED, WRAP2_FILTER, WRAP2_CAP = (2, 8, 32, 2, 6), 3, 1, 8
CASES = [("c2n6e2pent", 8), ("wrap", 8), ("wrap2", WRAP2_CAP), ("cfg4s1", 8), ("cfg4s4", 8), ("cfg4s9", 8), ("cfg4s9", 16)]
IDS = ["%s-%d" % c for c in CASES]
PASSES = [1, 2, 8]
_SOLVED, _CLIMB, _REPLAY, _PARAMS = {}, {}, {}, {}


def _params(name):
    """shared and left unchanged"""
    if name == "wrap2":
        if name not in _PARAMS:
            _PARAMS[name] = synthetic.generate(WRAP2_CFG, WRAP2_SEED, gap=1e-4)
        return _PARAMS[name]
    return _filter_params(name)


def _fam(name):
    return WRAP2_FILTER if name == "wrap2" else FILTER


def _site_of(dims, first):
    """the site (in the order of pool_site) that holds decision byte `first`"""
    Cn, N, O = dims
    f_env = Cn * N; f_obs = f_env + 5 * Cn * N; f_c2c = f_obs + 5 * Cn * O * N
    if first < f_env:
        return first // N
    if first < f_obs:
        return Cn + ((first - f_env) // (5 * N)) * 5 + (first - f_env) % 5
    if first < f_c2c:
        return 6 * Cn + ((first - f_obs) // (5 * N)) * 5 + (first - f_obs) % 5
    return 6 * Cn + 5 * Cn * O + ((first - f_c2c) // (4 * N)) * 4 + (first - f_c2c) % 4


def _fresh(name, cap):
    w = P.CplexWrapper(); w.resetParameters(_params(name))
    assert w.setSolutionPool(cap) == 0 and w.setSolutionPoolFilter(_fam(name)) == 0
    s = _as_found(w, w.callCplex())
    assert s["status"] == P.OptimizationStatus.SUCCESS and s["n"] >= 1, (name, cap, s["status"], s["n"])
    return s


def _solved(name, cap):
    """a solve whose pool nothing touches"""
    if (name, cap) not in _SOLVED:
        _SOLVED[(name, cap)] = _fresh(name, cap)
    return _SOLVED[(name, cap)]


def _timing(w):
    t = (P.wrapper.C.c_double * 6)()
    assert w._L.miqp_solver_last_timing(w._h, t) == 0
    return list(t)


def _climb(name, cap, passes):
    """a fresh solve and improveSolutionPool(passes) behind it: the pool as found, the call's arrays and timing, the pool it leaves"""
    key = (name, cap, passes)
    if key not in _CLIMB:
        s = _fresh(name, cap)
        w = s["w"]
        rc, before, after, moves, status = w.improveSolutionPool(passes)
        t = _timing(w)
        n = w.solutionPoolCount()
        _CLIMB[key] = dict(w=w, solved=s, rc=rc, before=before, after=after, moves=moves, status=status, timing=t, err=w.lastError(), n=n,
                           found=w.solutionPoolFound(), dec=[w.solutionPoolFoundDecisions(k) for k in range(n)])
        print("IMPROVE %s capacity %d passes %d: rc %d, passes run %d, neighbours %d, iterations %d, still moving %d, device %.1f ms of %.1f ms"
              % (name, cap, passes, rc, t[2], t[3], t[4], t[5], 1e3 * t[1], 1e3 * t[0]))
        for k in range(len(moves)):
            if moves[k] > 0:
                print("IMPROVE %s capacity %d passes %d: entry %d found %.6f tight %.6f -> %.6f in %d moves" % (name, cap, passes, k, s["found"][k], before[k], after[k], moves[k]))
    return _CLIMB[key]


def _accepts(cur, obj):
    """the acceptance rule: below the current objective by more than 1e-9 (1 + |current|), every operation rounded on its own"""
    return np.float64(cur) - np.float64(obj) > np.float64(1e-9) * (np.float64(1.0) + abs(np.float64(cur)))


def _replay(name, cap):
    """the climb as a host loop over pool_moves and solveDecisions, up to 8 passes: `before`, `status` and the state behind every pass that ran"""
    if (name, cap) in _REPLAY:
        return _REPLAY[(name, cap)]
    s = _solved(name, cap)
    Cn, N, O = s["dims"]
    w = P.CplexWrapper(); w.resetParameters(_params(name))
    cur = [d.copy() for d in s["dec"]]
    rc, st, obj, viol, it, route, best = w.solveDecisions(np.stack(cur))
    assert rc == 0
    before, status, curobj, moves = obj.copy(), (st != 0).astype(np.int32), obj.copy(), np.zeros(len(cur), dtype=np.int32)
    active = [x == 0 for x in st]
    states = {0: dict(after=curobj.copy(), moves=moves.copy(), dec=[d.copy() for d in cur], passes=0, neighbours=0, iterations=0, moved=False)}
    neighbours = iterations = largest = 0
    sites = []   # per pass and entry: the site of every move
    for p in range(1, 9):
        lists = [P.pool_moves(Cn, N, O, _fam(name), cur[k]) if active[k] else np.zeros((0, 4), dtype=np.int32) for k in range(len(cur))]
        total = sum(len(m) for m in lists)
        if total == 0:
            break
        sites.append([[_site_of(s["dims"], int(f)) for f in m[:, 0]] for m in lists])
        recs = np.empty((total, cur[0].size), dtype=np.int8)
        q = 0
        for k, mv in enumerate(lists):
            for first, stride, count, value in mv:
                recs[q] = cur[k]
                recs[q, first:first + count * stride:stride] = value
                q += 1
        rc, st, obj, viol, it, route, best = w.solveDecisions(recs)
        assert rc == 0 and not (st == 2).any()
        print("REPLAY %s capacity %d pass %d: %d neighbours%s" % (name, cap, p, total, " (more than one chunk)" if total > P.fixed_batch_chunk() else ""))
        neighbours += total; iterations += int(it.sum()); largest = max(largest, total)
        q, moved = 0, False
        for k, mv in enumerate(lists):
            bj = -1
            for j in range(len(mv)):
                if st[q + j] == 0 and (bj < 0 or obj[q + j] < obj[q + bj]):
                    bj = j
            active[k] = bool(bj >= 0 and _accepts(curobj[k], obj[q + bj]))
            if active[k]:
                first, stride, count, value = mv[bj]
                cur[k][first:first + count * stride:stride] = value
                curobj[k] = obj[q + bj]; moves[k] += 1; moved = True
            q += len(mv)
        states[p] = dict(after=curobj.copy(), moves=moves.copy(), dec=[d.copy() for d in cur], passes=p, neighbours=neighbours, iterations=iterations, moved=moved)
        if not moved:
            break
    _REPLAY[(name, cap)] = (before, status, states, largest, sites)
    return _REPLAY[(name, cap)]


def _same_solve(a, b, what):
    assert a["status"] == b["status"] == P.OptimizationStatus.SUCCESS, what
    assert _bytes(a["rec"], a["props"].objective) == _bytes(b["rec"], b["props"].objective), what
    assert a["props"].nodes == b["props"].nodes and a["n"] == b["n"], what
    assert a["found"].tobytes() == b["found"].tobytes(), what
    for k in range(a["n"]):
        assert a["dec"][k].tobytes() == b["dec"][k].tobytes(), (what, k)


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_solve_is_untouched(name, cap):
    """what a wrapper holds of its solve is the same bytes before and after another wrapper of the instance improved its pool, the solve of that
    other wrapper was the same solve, and a solve BEHIND an improve on the same wrapper equals a fresh one"""
    a = _solved(name, cap)
    c = _climb(name, cap, 8)
    _same_solve(a, c["solved"], (name, cap, "the climbing wrapper's own solve"))
    _same_solve(a, _as_found(a["w"], a["status"]), (name, cap, "the untouched wrapper behind the other's climb"))
    w = _climb(name, cap, 2)["w"]
    _same_solve(a, _as_found(w, w.callCplex()), (name, cap, "a solve behind an improve"))
    _CLIMB.pop((name, cap, 2))   # (its pool is the new solve's now)


@pytest.mark.parametrize("name", ["c2n6e2pent", "wrap", "cfg4s1", "cfg4s4", "cfg4s9"])
def test_solve_decisions(name):
    """solveDecisions of the found records: independent of the position (reversed; 1 500 records across the chunk boundary, every copy the bytes of
    the first), an out-of-range byte refuses that entry alone, and the labels solveSolutionPool ended on for an entry - those of its solutionPoolRecord, and
    where they did not move the search's own - are answered as that call and as solveFixedBatch of the record answer them.  (On these instances the
    search's labels always move in the first re-labelling pass: the count is printed.)"""
    s = _fresh(name, 8)
    w, n = s["w"], s["n"]
    recs = np.stack(s["dec"])
    w2 = P.CplexWrapper(); w2.resetParameters(_params(name))
    base = w2.solveDecisions(recs)
    assert base[0] == 0 and (base[1] != 2).all() and (base[1] == 0).any(), (name, base[0], list(base[1]))
    rev = w2.solveDecisions(recs[::-1])
    for a, b in zip(base[1:6], rev[1:6]):
        assert a.tobytes() == b[::-1].tobytes(), name
    feas = [k for k in range(n) if base[1][k] == 0]
    assert base[6] == min(feas, key=lambda k: (base[2][k], k)) and rev[6] == min(feas, key=lambda k: (base[2][k], -k)) * -1 + n - 1
    many = w2.solveDecisions(recs[np.arange(1500) % n])
    assert many[0] == 0 and 1500 > P.fixed_batch_chunk()
    for a, b in zip(base[1:6], many[1:6]):
        assert b.tobytes() == a[np.arange(1500) % n].tobytes(), name
    bad = np.concatenate([recs, recs[:1]])
    bad[n, 1] = 127   # step 1 of car 0: no car has that many possible regions
    out = w2.solveDecisions(bad)
    assert out[0] == 0 and out[1][n] == 2 and np.isnan(out[2][n]) and out[5][n] == -1
    for a, b in zip(base[1:6], out[1:6]):
        assert a.tobytes() == b[:n].tobytes(), name
    st, obj, viol, it, route = w.solveSolutionPool()
    same = 0
    for k in range(w.solutionPoolCount()):
        rc, rec = w.solutionPoolRecord(k)
        if rc != 0:
            continue
        # the labels the refinement's last pass solved this entry with are those of its record (families 31: the signature is the bytes)
        labels = [w.poolSignature(rec, 31)]
        d = w.solutionPoolFoundDecisions(k)
        if labels[0].tobytes() == d.tobytes():   # the search's own labels did not move: its record as found is answered the same
            same += 1; labels.append(d)
        fb = w2.solveFixedBatch([rec])
        for lab in labels:
            one = w2.solveDecisions(lab[None, :])
            for a, b, c in zip(one[1:6], fb[0:5], (st, obj, viol, it, route)):
                assert a.tobytes() == b.tobytes() == c[k:k + 1].tobytes(), (name, k)
    print("DECISIONS %s: %d of %d entries kept the search's labels in solveSolutionPool" % (name, same, w.solutionPoolCount()))


def test_the_wrapping_instance_has_moves_past_lane_63():
    """a condition on the inputs, so that the replay comparison below pins the second 64-site block of pool_moves_kernel - its part of the scan, the
    carry between the blocks and the table offsets of sites 64 .. 75: in some pass an entry of wrap2 has moves on a site >= 64 AND on a site < 64
    (its numbering crosses the block).  A wrong count, carry or offset there puts other moves into the table: other neighbours are solved, and the
    comparison of the neighbour count, of the iteration sum over all neighbours (out[3], out[4]) and of the records left sees it"""
    s = _solved("wrap2", WRAP2_CAP)
    Cn, N, O = s["dims"]
    assert 6 * Cn + 5 * Cn * O + 4 * (Cn * (Cn - 1) // 2) == 76
    before, status, states, _, sites = _replay("wrap2", WRAP2_CAP)
    crossing = [(p + 1, k, len(e), sum(1 for x in e if x >= 64)) for p, entries in enumerate(sites) for k, e in enumerate(entries) if e and min(e) < 64 <= max(e)]
    print("WRAP2 seed %d capacity %d: (pass, entry, moves, of which on sites >= 64) %s" % (WRAP2_SEED, WRAP2_CAP, crossing))
    assert crossing
    changed = set()
    for p in range(1, max(states) + 1):
        for k in range(len(before)):
            for q in np.nonzero(states[p]["dec"][k] != states[p - 1]["dec"][k])[0]:
                changed.add(_site_of(s["dims"], int(q)))
    print("WRAP2 sites whose bytes the climb changed: %s" % sorted(changed))


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_climb_is_its_host_replay(name, cap, passes):
    before, status, states, _, _ = _replay(name, cap)
    c = _climb(name, cap, passes)
    e = states[min(passes, max(states))]
    assert c["rc"] == int((e["moves"] > 0).sum()) and c["n"] == len(before) == c["solved"]["n"]
    assert c["before"].tobytes() == before.tobytes(), (list(c["before"]), list(before))
    assert c["status"].tobytes() == status.tobytes()
    live = status == 0
    assert c["after"][live].tobytes() == e["after"][live].tobytes(), (list(c["after"]), list(e["after"]))
    assert c["after"][~live].tobytes() == before[~live].tobytes() and not c["moves"][~live].any()
    assert c["moves"].tobytes() == e["moves"].tobytes(), (list(c["moves"]), list(e["moves"]))
    for k in range(c["n"]):
        assert c["dec"][k].tobytes() == e["dec"][k].tobytes(), (name, cap, passes, k)
    t = c["timing"]
    still = 1 if e["passes"] == passes and e["moved"] else 0
    assert (t[2], t[3], t[4], t[5]) == (e["passes"], e["neighbours"], e["iterations"], still), (t, e["passes"], e["neighbours"], e["iterations"], still)
    assert ("still moved" in c["err"]) == bool(still)


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_properties(name, cap):
    c = _climb(name, cap, 8)
    s = c["solved"]
    Cn, N, O = s["dims"]
    assert c["n"] == s["n"]
    for k in range(c["n"]):
        assert c["after"][k] <= c["before"][k]
        assert (np.float64(c["after"][k]).tobytes() == np.float64(c["before"][k]).tobytes()) == (c["moves"][k] == 0), (name, k)
        assert (c["dec"][k].tobytes() == s["dec"][k].tobytes()) == (c["moves"][k] == 0), (name, k)
        assert P.pool_signature(Cn, N, O, _fam(name), c["dec"][k]).tobytes() == P.pool_signature(Cn, N, O, _fam(name), s["dec"][k]).tobytes(), (name, k)
        assert np.float64(c["found"][k]).tobytes() == np.float64(c["after"][k] if c["status"][k] == 0 else s["found"][k]).tobytes(), (name, k)
    # entry 0 as found is the incumbent's own record: pool_read_back puts it there, and test_pool_filter_gpu.py (test_refinement_under_the_filter:
    # entry 0 has the incumbent's binaries) ties it to the result record.  The canonical labels of the RESULT record can name another alternative
    # that holds as well, so here the climbed entry 0 is compared with entry 0 of a solve nothing touched: the climb left it in that class
    assert P.pool_signature(Cn, N, O, _fam(name), c["dec"][0]).tobytes() == P.pool_signature(Cn, N, O, _fam(name), _solved(name, cap)["dec"][0]).tobytes(), name
    if name in ("c2n6e2pent", "wrap", "wrap2") and c["timing"][5] == 0:   # a local optimum, asserted directly: no kept move of a final record improves it by more than the allowance
        w2 = P.CplexWrapper(); w2.resetParameters(_params(name))
        for k in range(c["n"]):
            mv = P.pool_moves(Cn, N, O, _fam(name), c["dec"][k])
            if c["status"][k] != 0 or len(mv) == 0:
                continue
            recs = np.repeat(c["dec"][k][None, :], len(mv), axis=0)
            for q, (first, stride, count, value) in enumerate(mv):
                recs[q, first:first + count * stride:stride] = value
            rc, st, obj, viol, it, route, best = w2.solveDecisions(recs)
            assert rc == 0
            for q in range(len(mv)):
                assert st[q] != 0 or not _accepts(c["after"][k], obj[q]), (name, k, q, c["after"][k], obj[q])


def test_it_does_something():
    """a condition on the inputs: on at least one instance at least one entry moves (cfg4 seed 9, whose filtered pool holds leaves far above the
    incumbent, is the expected one)"""
    moved = {}
    for name, cap in CASES:
        c = _climb(name, cap, 8)
        moved[(name, cap)] = [(k, float(c["before"][k]), float(c["after"][k]), int(c["moves"][k])) for k in range(c["n"]) if c["moves"][k] > 0]
    print("IMPROVE moved", moved)
    assert any(moved.values()), moved


@pytest.mark.parametrize("name,cap", [CASES[0], CASES[1], CASES[2], CASES[5]], ids=[IDS[0], IDS[1], IDS[2], IDS[5]])
def test_reproducible(name, cap):
    a = _climb(name, cap, 8)
    _CLIMB.pop((name, cap, 8))
    b = _climb(name, cap, 8)
    for n in ("before", "after", "moves", "status", "found"):
        assert a[n].tobytes() == b[n].tobytes(), (name, n)
    assert a["rc"] == b["rc"] and a["n"] == b["n"] and a["timing"][2:] == b["timing"][2:]
    for k in range(a["n"]):
        assert a["dec"][k].tobytes() == b["dec"][k].tobytes(), (name, k)


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_refinement_behind_the_climb(name, cap):
    """solveSolutionPool behind the climb: every surviving entry comes out no worse than the climb left it (the QP of the re-labelled record contains
    the improved optimum), and every record certifies"""
    c = _climb(name, cap, 8)
    w = c["w"]
    st, obj, viol, it, route = w.solveSolutionPool()
    found = w.solutionPoolFound()
    assert len(obj) == w.solutionPoolCount() == len(found) >= 1
    alive = {np.float64(a).tobytes() for a, x in zip(c["after"], c["status"]) if x == 0}
    for k in range(len(obj)):
        rc, rec = w.solutionPoolRecord(k)
        if np.float64(found[k]).tobytes() not in alive:
            continue   # (an entry the climb left as it was found: not feasible at the tight tolerance)
        assert st[k] == 0 and rc == 0, (name, k, st[k], rc)
        assert obj[k] <= found[k] * (1 + OBJ_RTOL), (name, k, obj[k], found[k])
        cert = w.certify(rec)
        assert cert.status == 0 and cert.max_violation < 1e-5, (name, k, cert)
    _CLIMB.pop((name, cap, 8))   # (its pool is the refined one now)

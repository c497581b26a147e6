"""The kept manoeuvres of one planning cycle carried into the pool of the next on the device (carrySolutionPool).

Cases, under filter 12: c2n6e2pent at capacity 8 (N = 6, the smallest shape), wrap at capacity 8 (76 sites: the shift kernel's loop over the sites
wraps past 64 lanes), cfg4 seeds 12, 10 and 5 at capacity 16.  Per case the SOURCE is solved and explored (exploreSolutionPool(settled=True)); the
DESTINATION is synthetic.advance of the source's parameters along the source's solution, solved on a fresh wrapper.  Every solve and every call runs
once on a fresh wrapper and is kept for the tests that share it.

The reference of the call is its HOST REPLAY (_replay), which uses neither new kernel: pool_shift per source entry with the maps restated in Python,
solveDecisions for the first solves, ONE settleDecisions call over the destination's own entries and the mappable shifted records, pool_signature
for both signatures, and the visiting order, the cost cap and the place count restated.  Both sides are bit for bit.
For the record (one MI355X, shift 1, no cap): the sources keep 8, 1, 5, 10 and 16 entries and the replay admits 0, 0, 2, 0 and 8 of them - on
c2n6e2pent, wrap and seed 10 every source entry is infeasible one step on (status 1) or of a class the new solve found itself (3, 4); into an EMPTY
pool c2n6e2pent carries 1 and seed 12 carries 3.  Status 1 occurs in four cases, status 2 is forced on c2n6e2pent (7 of 8 records).
All tests here need a real MI355X: run with  python -m pytest tests/test_pool_carry_gpu.py -m gpu -s."""
import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import PoolCarryC
from test_pool_carry_cpu import _region_map
from test_pool_explore_gpu import _same_solve, _timing, _within
from test_pool_filter_gpu import FILTER, _as_found, _params

pytestmark = pytest.mark.gpu

CASES = [("c2n6e2pent", 8), ("wrap", 8), ("cfg4s12", 16), ("cfg4s10", 16), ("cfg4s5", 16)]
IDS = ["%s-%d" % c for c in CASES]
_SRC, _DSTP, _DST, _CARRIED, _REPLAY = {}, {}, {}, {}, {}
NAN = float("nan")


def _source(name, cap):
    """the source of a case: solved, explored, its pool as it stands then (shared and left unchanged)"""
    if (name, cap) not in _SRC:
        w = P.CplexWrapper(); w.resetParameters(_params(name))
        assert w.setSolutionPool(cap) == 0 and w.setSolutionPoolFilter(FILTER) == 0
        st = w.callCplex()
        assert st == P.OptimizationStatus.SUCCESS, (name, st)
        rec = w.getRawResults()
        rc, added = w.exploreSolutionPool(settled=True)
        assert rc >= 0
        s = _as_found(w, st)
        s["rec"], s["explored"] = rec, rc
        _SRC[(name, cap)] = s
        print("CARRY source %s capacity %d: %d entries (%d explored), found %s" % (name, cap, s["n"], rc, list(s["found"])))
    return _SRC[(name, cap)]


def _free_region(p, c):
    """the lowest region number that is not possible for car c: below the highest possible one (the possible regions wrap around number 0)"""
    row = np.asarray(p.possible_region).reshape(p.NumCars, -1)[c]
    free = int(np.flatnonzero(row != 1)[0])
    assert (np.flatnonzero(row == 1) > free).any()
    return free


def _used_regions(s, p, shift):
    """per car the region NUMBERS the source's entries use at the steps a shift by `shift` reads"""
    Cn, N, O = s["dims"]
    poss = np.asarray(p.possible_region).reshape(Cn, -1)
    used = []
    for c in range(Cn):
        nums = np.flatnonzero(poss[c] == 1)
        used.append({int(nums[int(d[c * N + i]) >> 2]) for d in s["dec"] for i in range(1 + shift, N) if d[c * N + i] >= 0})
    return used


def _dst_params(name, cap, shift, variant):
    """the destination's parameters: advanced along the source's solution; `extra`: one more possible region for car 0, so that the region map is
    not the identity; `without`: a region the source's entries use (not the destination's initial one) is not possible: unmappable records"""
    key = (name, cap, shift, variant)
    if key not in _DSTP:
        s = _source(name, cap)
        p = _params(name)
        if variant == "extra":
            q = synthetic.advance(p, s["rec"], shift, extra_possible=[(0, _free_region(p, 0))])
        else:
            q = synthetic.advance(p, s["rec"], shift)
        if variant == "without":
            used = _used_regions(s, p, shift)
            pick = [(c, j) for c in range(len(used)) for j in sorted(used[c]) if j != int(q.initial_region[c]) - 1]
            if not pick:
                _DSTP[key] = None
                return None
            poss = np.array(q.possible_region).reshape(len(used), -1); poss[pick[0][0], pick[0][1]] = 0
            q.possible_region = poss
        _DSTP[key] = q
    return _DSTP[key]


def _fresh_dst(name, cap, shift, variant, dcap=None, solve=True):
    w = P.CplexWrapper(); w.resetParameters(_dst_params(name, cap, shift, variant))
    assert w.setSolutionPool(cap if dcap is None else dcap) == 0 and w.setSolutionPoolFilter(FILTER) == 0
    if not solve:
        assert w._loaded()
        return dict(w=w, n=0, found=np.zeros(0), dec=[], dims=_source(name, cap)["dims"], status=None)
    s = _as_found(w, w.callCplex())
    assert s["status"] == P.OptimizationStatus.SUCCESS and s["n"] >= 1, (name, shift, variant, s["status"])
    return s


def _dst(name, cap, shift, variant, dcap=None, solve=True):
    """a destination solve whose pool nothing touches"""
    key = (name, cap, shift, variant, dcap, solve)
    if key not in _DST:
        _DST[key] = _fresh_dst(name, cap, shift, variant, dcap, solve)
    return _DST[key]


def _pool(w):
    n = w.solutionPoolCount()
    return dict(n=n, found=w.solutionPoolFound(), dec=[w.solutionPoolFoundDecisions(k) for k in range(n)])


def _carried(name, cap, shift=1, max_rel=-1.0, variant="plain", dcap=None, solve=True):
    """a fresh destination and carrySolutionPool from the case's source behind it"""
    key = (name, cap, shift, max_rel, variant, dcap, solve)
    if key not in _CARRIED:
        d = _fresh_dst(name, cap, shift, variant, dcap, solve)
        w = d["w"]
        t0 = _timing(w)
        rc, out = w.carrySolutionPool(_source(name, cap)["w"], shift, max_rel)
        t = _timing(w)
        _CARRIED[key] = dict(w=w, solved=d, rc=rc, out=out, timing=t, timing_before=t0, err=w.lastError(), kernels=P.pool_carry_last(), **_pool(w))
        print("CARRY %s capacity %d shift %d max_rel %g %s: rc %d, statuses %s, %d -> %d entries, groups %d solves %d iterations %d still %d, device %.2f ms of %.2f ms (shift %.3f, admit %.3f)"
              % (name, cap, shift, max_rel, variant, rc, [o["status"] for o in out], d["n"], _CARRIED[key]["n"], t[2], t[3], t[4], t[5], 1e3 * t[1], 1e3 * t[0],
                 1e3 * _CARRIED[key]["kernels"][0], 1e3 * _CARRIED[key]["kernels"][1]))
    return _CARRIED[key]


def _env_map(ps, pd):
    return np.array([next((f for f, b in enumerate(pd.MultiEnvironmentConvexPolygon) if np.array_equal(np.asarray(a), np.asarray(b))), -1)
                     for a in ps.MultiEnvironmentConvexPolygon], dtype=np.int32)


def _replay(name, cap, shift=1, max_rel=-1.0, variant="plain", dcap=None, solve=True):
    """the call as host code over pool_shift, solveDecisions, settleDecisions and pool_signature"""
    key = (name, cap, shift, max_rel, variant, dcap, solve)
    if key in _REPLAY:
        return _REPLAY[key]
    s, d = _source(name, cap), _dst(name, cap, shift, variant, dcap, solve)
    Cn, N, O = s["dims"]
    K = cap if dcap is None else dcap
    ps, pd = _params(name), _dst_params(name, cap, shift, variant)
    rm, em = _region_map(np.asarray(ps.possible_region).reshape(Cn, -1), np.asarray(pd.possible_region).reshape(Cn, -1)), _env_map(ps, pd)
    w = P.CplexWrapper(); w.resetParameters(pd)
    crm, cem = w.poolCarryMaps(s["w"])
    assert crm.tobytes() == rm.tobytes() and cem.tobytes() == em.tobytes()
    ns, n0 = min(s["n"], 16), d["n"]
    shifted = [P.pool_shift(Cn, N, O, shift, x, rm, em) for x in s["dec"][:ns]]
    ok = [k for k in range(ns) if shifted[k][0]]
    out = [dict(status=2, place=-1, solves=0, iterations=0, objective=NAN) for k in range(ns)]
    dec, found = [x.copy() for x in d["dec"]], [float(x) for x in d["found"]]
    groups = solves_all = iters_all = still = 0
    if n0 >= K or ns == 0:
        e = dict(rc=0, out=[], dec=dec, found=found, timing=None, mappable=ok)
        _REPLAY[key] = e
        return e
    sig = lambda x: P.pool_signature(Cn, N, O, FILTER, x).tobytes()   # noqa: E731
    sigs = [sig(x) for x in dec]
    ssigs = []
    if n0 + len(ok) > 0:
        if ok:
            rc, st1, obj1, _, it1, _, _ = w.solveDecisions(np.stack([shifted[k][1] for k in ok]))
            assert rc == 0 and not (st1 == 2).any()
        rc, st, obj, _, it, _, _, settled, solves = w.settleDecisions(np.stack(dec + [shifted[k][1] for k in ok]))
        assert rc == 0 and not (st == 2).any() and (solves != 0).all()
        t = _timing(w)
        groups, solves_all, iters_all = t[2], t[3], t[4]
        ssigs = [sig(settled[j]) if st[j] == 0 else None for j in range(n0)]
        still = int((solves[n0:] < 0).any())
    first = {}
    for a, k in enumerate(ok):
        first[k] = (int(st1[a]), float(obj1[a]), int(it1[a]))
        out[k] = dict(status=1, place=-1, solves=abs(int(solves[n0 + a])), iterations=int(it1[a]), objective=float(obj1[a]))
    n, obj0 = n0, (found[0] if n0 else None)
    for a, k in sorted(((a, k) for a, k in enumerate(ok) if first[k][0] == 0), key=lambda ak: (first[ak[1]][1], ak[1])):
        o = first[k][1]
        if n > 0 and not _within(obj0, o, max_rel):
            out[k]["status"] = 5
        elif sig(shifted[k][1]) in sigs:
            out[k]["status"] = 3
        elif st[n0 + a] != 0 or sig(settled[n0 + a]) in [x for x in ssigs if x is not None]:
            out[k]["status"] = 4
        elif n >= K:
            out[k]["status"] = 6
        else:
            out[k]["status"], out[k]["place"] = 0, n
            dec.append(shifted[k][1].copy()); found.append(o); sigs.append(sig(shifted[k][1])); ssigs.append(sig(settled[n0 + a]))
            if n == 0:
                obj0 = o
            n += 1
    e = dict(rc=n - n0, out=out, dec=dec, found=found, timing=(groups, solves_all, iters_all, still), mappable=ok)
    print("REPLAY %s capacity %d shift %d max_rel %g %s: %d source entries, %d mappable, statuses %s, admitted %d" % (name, cap, shift, max_rel, variant, ns, len(ok), [o["status"] for o in out], n - n0))
    _REPLAY[key] = e
    return e


def _same_as_replay(c, e, what):
    s = c["solved"]
    assert c["rc"] == e["rc"] and c["n"] == len(e["dec"]) == s["n"] + c["rc"], (what, c["rc"], e["rc"])
    assert len(c["out"]) == len(e["out"]), what
    for a, b in zip(c["out"], e["out"]):
        assert {k: v for k, v in a.items() if k != "objective"} == {k: v for k, v in b.items() if k != "objective"}, (what, a, b)
        assert np.float64(a["objective"]).tobytes() == np.float64(b["objective"]).tobytes() or (a["status"] == b["status"] == 2 and np.isnan(a["objective"])), (what, a, b)
    assert c["found"].tobytes() == np.array(e["found"], dtype=np.float64).tobytes(), (what, list(c["found"]), e["found"])
    for k in range(c["n"]):
        assert c["dec"][k].tobytes() == e["dec"][k].tobytes(), (what, k)
    for k in range(s["n"]):   # old entries are the same bytes in the same places
        assert c["dec"][k].tobytes() == s["dec"][k].tobytes() and np.float64(c["found"][k]).tobytes() == np.float64(s["found"][k]).tobytes(), (what, k)
    if e["timing"] is None:   # (no device work: the timing is still what it was)
        assert c["timing"] == c["timing_before"] and c["err"] == ""
    else:
        assert tuple(c["timing"][2:6]) == tuple(e["timing"]), (what, c["timing"], e["timing"])
        assert ("still moved" in c["err"]) == bool(e["timing"][3])


def test_it_does_something():
    """conditions on the inputs, checked on the REPLAY: it admits on at least two of the five cases, and a carried record that is not feasible on
    the destination occurs.  What each case gives is printed for the record"""
    admitted, statuses = {}, set()
    for name, cap in CASES:
        e = _replay(name, cap)
        admitted[(name, cap)] = e["rc"]
        statuses |= {o["status"] for o in e["out"]}
    print("REPLAY admitted %s, statuses seen %s" % (admitted, sorted(statuses)))
    assert sum(1 for v in admitted.values() if v > 0) >= 2, admitted
    assert 1 in statuses, statuses


@pytest.mark.parametrize("max_rel", [-1.0, 0.5])
@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_carry_is_its_host_replay(name, cap, max_rel):
    _same_as_replay(_carried(name, cap, 1, max_rel), _replay(name, cap, 1, max_rel), (name, cap, max_rel))


@pytest.mark.parametrize("name,cap", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_a_shift_of_two_steps(name, cap):
    _same_as_replay(_carried(name, cap, 2), _replay(name, cap, 2), (name, cap, "shift 2"))


@pytest.mark.parametrize("name,cap", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_a_region_map_that_is_not_the_identity(name, cap):
    s = _source(name, cap)
    e = _replay(name, cap, 1, -1.0, "extra")
    rm, _ = _dst(name, cap, 1, "extra")["w"].poolCarryMaps(s["w"])
    assert not np.array_equal(rm[0], np.arange(rm.shape[1]))
    _same_as_replay(_carried(name, cap, 1, -1.0, "extra"), e, (name, cap, "extra possible region"))


def test_unmappable_records():
    """a destination without one region the source's entries use: those records are status 2, the others go on as ever"""
    seen = 0
    for name, cap in CASES:
        if _dst_params(name, cap, 1, "without") is None:
            continue
        e = _replay(name, cap, 1, -1.0, "without")
        assert any(o["status"] == 2 for o in e["out"]), (name, [o["status"] for o in e["out"]])
        c = _carried(name, cap, 1, -1.0, "without")
        _same_as_replay(c, e, (name, cap, "without a region"))
        for o in c["out"]:
            if o["status"] == 2:
                assert np.isnan(o["objective"]) and (o["place"], o["solves"], o["iterations"]) == (-1, 0, 0)
        seen += 1
        break
    assert seen == 1


def test_a_full_destination():
    name, cap = CASES[2]
    e = _replay(name, cap, 1, -1.0, "plain", 1)
    c = _carried(name, cap, 1, -1.0, "plain", 1)
    assert c["solved"]["n"] == 1 and c["rc"] == 0 and c["out"] == [] and e["timing"] is None
    _same_as_replay(c, e, (name, "capacity 1"))


@pytest.mark.parametrize("name,cap", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_an_empty_destination(name, cap):
    """a destination with its instance loaded, capacity and filter set and no solve: entry 0 afterwards is the best feasible carried record,
    whatever the cap"""
    for max_rel in (-1.0, 0.0):
        e = _replay(name, cap, 1, max_rel, "plain", None, False)
        c = _carried(name, cap, 1, max_rel, "plain", None, False)
        _same_as_replay(c, e, (name, cap, "empty", max_rel))
        feasible = [o for o in c["out"] if o["status"] not in (1, 2)]
        assert feasible and c["rc"] >= 1 and c["n"] == c["rc"]
        best = min(range(len(c["out"])), key=lambda k: (c["out"][k]["objective"], k) if c["out"][k]["status"] not in (1, 2, 4) else (np.inf, k))
        assert c["out"][best]["status"] == 0 and c["out"][best]["place"] == 0
        assert np.float64(c["found"][0]).tobytes() == np.float64(c["out"][best]["objective"]).tobytes()
        if max_rel == 0.0:   # everything dearer than entry 0 is beyond the cap
            assert all(o["status"] != 0 or o["objective"] <= c["found"][0] for o in c["out"])
    # a solve behind it is a fresh one
    w = _carried(name, cap, 1, -1.0, "plain", None, False)["w"]
    _same_solve(_dst(name, cap, 1, "plain"), _as_found(w, w.callCplex()), (name, "a solve behind a carry into an empty pool"))
    _CARRIED.pop((name, cap, 1, -1.0, "plain", None, False))


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_source_is_only_read_and_the_call_is_reproducible(name, cap):
    s = _source(name, cap)
    a = _carried(name, cap)
    _CARRIED.pop((name, cap, 1, -1.0, "plain", None, True))
    b = _carried(name, cap)
    assert a["rc"] == b["rc"] and a["n"] == b["n"] and a["timing"][2:] == b["timing"][2:] and a["found"].tobytes() == b["found"].tobytes() and a["err"] == b["err"]
    assert [sorted((k, np.float64(v).tobytes() if k == "objective" else v) for k, v in x.items()) for x in a["out"]] == \
           [sorted((k, np.float64(v).tobytes() if k == "objective" else v) for k, v in x.items()) for x in b["out"]]
    for k in range(a["n"]):
        assert a["dec"][k].tobytes() == b["dec"][k].tobytes(), (name, k)
    now = _pool(s["w"])
    assert now["n"] == s["n"] and now["found"].tobytes() == s["found"].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(now["dec"], s["dec"]))


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_refinement_climb_and_solve_behind_the_carry(name, cap):
    """solveSolutionPool behind the call leaves what it leaves of the destination's own pool and every carried entry; its records certify; the climb
    runs on the larger pool; a solve behind the call equals a fresh one"""
    c = _carried(name, cap)
    _CARRIED.pop((name, cap, 1, -1.0, "plain", None, True))   # (its pool is the refined one from here on)
    w = c["w"]
    twin = _fresh_dst(name, cap, 1, "plain")
    L0 = len(twin["w"].solveSolutionPool()[1])
    rc, before, after, moves, status = w.improveSolutionPool(8)
    assert rc >= 0 and len(before) == c["n"] == w.solutionPoolCount(), (name, rc)
    w2 = _carried(name, cap)["w"]   # (the climb moved entries: the refinement is checked on a pool as the carry left it)
    _CARRIED.pop((name, cap, 1, -1.0, "plain", None, True))
    st, obj, viol, it, route = w2.solveSolutionPool()
    assert len(obj) == w2.solutionPoolCount() == L0 + c["rc"], (name, len(obj), L0, c["rc"])
    for k in range(len(obj)):
        rc, rec = w2.solutionPoolRecord(k)
        assert (rc == 0) == (st[k] == 0), (name, k, rc, st[k])
        if rc == 0:
            cert = w2.certify(rec)
            assert cert.status == 0 and cert.max_violation < 1e-5, (name, k, cert)
    assert (st[L0:] == 0).all()   # (a carried entry has settled labels: its own QP is feasible)
    _same_solve(_dst(name, cap, 1, "plain"), _as_found(w2, w2.callCplex()), (name, cap, "a solve behind a carry"))
    _same_solve(_dst(name, cap, 1, "plain"), c["solved"], (name, cap, "the carrying wrapper's own solve"))


def test_a_cap_below_the_source_entries_is_refused():
    name, cap = CASES[2]
    s, d = _source(name, cap), _fresh_dst(name, cap, 1, "plain")
    out = (PoolCarryC * 16)()
    for o in out:
        o.status = 9
    before = _pool(d["w"])
    assert s["n"] >= 1 and d["w"]._L.miqp_solver_pool_carry(d["w"]._h, s["w"]._h, 1, -1.0, out, s["n"] - 1) == -2
    after = _pool(d["w"])
    assert [o.status for o in out] == [9] * 16 and after["n"] == before["n"] and after["found"].tobytes() == before["found"].tobytes()

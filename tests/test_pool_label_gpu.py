"""The canonical labels of solved nodes written on the device (canonicalDecisions: pool_label_kernel) and the explore that admits a manoeuvre only
when its own labels are new (exploreSolutionPool(distinct=True)); DESIGN.md 6i.

a. The kernel against the host, directly: canonicalDecisions(records) row by row and byte for byte against poolSignature(fixedBatchRecord(k), 31) -
   with every family and exact timing that is the D bytes of fix_from_results of the host-built record - for every feasible k, all -1 for the others;
   `out` and `best` against solveDecisions of the same records bit for bit.  Records: the pool as found plus all pool_jumps neighbours of its entries
   on c2n6e2pent, wrap (76 sites: the lane loop wraps; more than one chunk of 1024 records, which pins the per-chunk path) and cfg4 seed 12; the relax
   levels (undecided car/car, obstacle and environment bytes), the jumps of the complete record and - on the instance with the obstacle made soft -
   the soft levels (byte L beside -1 and decided bytes) of c2n6e2pent, c1n21o (memory-backed route, N > 20) and c3n6o (three cars, three pairs);
   one hand-made batch that mixes a refused entry, infeasible entries and records with undecided bytes.
b. The distinct explore is its host replay (_replay_distinct: test_pool_explore_gpu._replay with pass 0 and the second signature, which is built from
   host-built records only - it uses neither new kernel), bit for bit, for 1 and 4 passes, without and with a cost cap.
c. Properties of the pool the call leaves.
d. What it is for, measured against the plain call on the same instances: merged(mode) = entries behind the explore - entries solveSolutionPool
   leaves.  Required: merged(distinct) <= merged(plain) on every case, the sum strictly smaller, and never fewer entries left in distinct mode.
   Measured on one MI355X (4 passes, no cap; entries found -> behind the explore -> left by the refinement):
   c2n6e2pent/8   plain  2 ->  8 ->  2, merged  6 | distinct  2 ->  8 ->  8, merged  0
   wrap/8         plain  1 ->  8 ->  1, merged  7 | distinct  1 ->  1 ->  1, merged  0
   cfg4s7/16      plain  1 -> 16 ->  1, merged 15 | distinct  1 ->  5 ->  1, merged  4
   cfg4s12/16     plain  1 -> 16 ->  3, merged 13 | distinct  1 ->  5 ->  5, merged  0
   cfg4s1/8       plain  2 ->  8 ->  2, merged  6 | distinct  2 ->  8 ->  2, merged  6
   cfg4s9/16      plain 16 -> 16 -> 13, merged  3 | distinct 16 -> 16 -> 13, merged  3   (a full pool: neither call does anything)
   in all         plain 50 merged                 | distinct 13 merged
   Where the distinct call still merges (seeds 7 and 1): the labels of a neighbour's own solution are new, but solved again under those labels it
   slides back to a kept entry's solution - the refinement iterates label-and-solve to a fixed point, the admission sees one step.
All tests here need a real MI355X: run with  python -m pytest tests/test_pool_label_gpu.py -m gpu -s."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import planner_miqp_amd as P
from test_pool_explore_gpu import CASES, FULL, IDS, MAX_REL, PASSES, _fresh, _same_solve, _solved, _timing, _within
from test_pool_filter_gpu import FILTER, _as_found, _params

pytestmark = pytest.mark.gpu

POOL_CASES = [("c2n6e2pent", 8), ("wrap", 8), ("cfg4s12", 16)]
ORACLE_SHAPES = ["c2n6e2pent", "c1n21o", "c3n6o"]
SOFT = [(n, m) for n, m in H.SOFT_CASES if n in ORACLE_SHAPES]
_EXPLORED, _REPLAY = {}, {}


def _wrapper(params):
    w = P.CplexWrapper(); w.resetParameters(params)
    return w


def _lines(w):
    d = (C.c_int * 6)()
    assert w._L.miqp_solver_get_dims(w._h, d) == 0
    return (d[0], d[1], d[4]), d[5]


def _neighbours(dims, lines, dec):
    """every pool_jumps neighbour of the record under the suite's filter"""
    out = []
    for first, stride, count, value in P.pool_jumps(dims[0], dims[1], dims[2], lines, FILTER, dec):
        r = dec.copy(); r[first:first + count * stride:stride] = value
        out.append(r)
    return out


def _host_labels(w, k, D):
    """row k of the last fixed call of w, host-built: poolSignature(fixedBatchRecord(k), 31); None when the entry is not feasible"""
    rc, rec = w.fixedBatchRecord(k)
    return w.poolSignature(rec, 31) if rc == 0 else None


def _check_labels(params, recs, tag):
    """a. for one batch; returns (status, canon)"""
    recs = np.ascontiguousarray(recs, dtype=np.int8)
    w = _wrapper(params)
    rc, st, obj, viol, it, route, best, canon = w.canonicalDecisions(recs)
    assert rc == 0 and canon.shape == recs.shape, (tag, rc, w.lastError())
    (Cn, N, O), _ = _lines(w)
    for k in range(len(recs)):
        want = _host_labels(w, k, recs.shape[1])
        assert (want is not None) == (st[k] == 0), (tag, k, st[k])
        if want is None or (recs[k][:Cn * N].reshape(Cn, N)[:, 1:] < 0).any():   # (an undecided region at a step >= 1: no labels, by definition)
            want = np.full(recs.shape[1], -1, dtype=np.int8)
        assert canon[k].tobytes() == want.tobytes(), (tag, k, [(int(q), int(canon[k][q]), int(want[q])) for q in np.flatnonzero(canon[k] != want)[:8]])
    w2 = _wrapper(params)
    ref = w2.solveDecisions(recs)
    assert ref[0] == rc and ref[6] == best, (tag, ref[6], best)
    for x, y, n in zip(ref[1:6], (st, obj, viol, it, route), ("status", "objective", "violation", "iterations", "route")):
        assert x.tobytes() == y.tobytes(), (tag, n)
    print("LABEL %s: %d records, %d feasible, %d infeasible, %d refused, %d distinct canonical rows among the feasible"
          % (tag, len(recs), int((st == 0).sum()), int((st == 1).sum()), int((st == 2).sum()), len({canon[k].tobytes() for k in range(len(recs)) if st[k] == 0})))
    return st, canon


@pytest.mark.parametrize("name,cap", POOL_CASES, ids=["%s-%d" % c for c in POOL_CASES])
def test_labels_of_the_pool_and_its_neighbours(name, cap):
    s = _solved(name, cap)
    recs = [d.copy() for d in s["dec"]]
    for d in s["dec"]:
        recs += _neighbours(s["dims"], s["lines"], d)
    if name == "wrap":   # more than one chunk of records: the neighbours of the neighbours, as far as needed
        for d in list(recs[s["n"]:]):
            if len(recs) > P.fixed_batch_chunk() + 64:
                break
            recs += _neighbours(s["dims"], s["lines"], d)
    st, canon = _check_labels(_params(name), np.stack(recs), "%s/%d" % (name, cap))
    assert (st == 0).sum() > s["n"] and not (st == 2).any()
    if name == "wrap":
        assert len(recs) > P.fixed_batch_chunk()   # (a condition on the inputs: more than one chunk)


def _decisions(w, record):
    return w.poolSignature(record, 31)


@pytest.mark.parametrize("name", ORACLE_SHAPES)
def test_labels_of_partial_records(oracle, name):
    """the relax levels of the shape's canonical complete record - undecided bytes of every leaf family - and the jumps of the complete one"""
    p, h, dims, rec = H.node_instance(oracle, name)
    w = _wrapper(p)
    levels = H.relax_levels(rec, 11)
    recs = [_decisions(w, r) for r, _ in levels.values()]
    recs += _neighbours((dims[0], dims[1], dims[4]), dims[5], recs[0])
    st, canon = _check_labels(p, np.stack(recs), name)
    assert (st[:len(levels)] == 0).all(), (name, list(st[:len(levels)]))   # (test_node_records_cpu.py: every level is feasible)
    if len(levels) > 1:
        und = np.stack(recs[:len(levels)]) < 0
        f_obs, f_c2c = dims[0] * dims[1] * 6, dims[0] * dims[1] * 6 + dims[0] * dims[4] * dims[1] * 5
        assert und[:, f_obs:f_c2c].reshape(len(levels), -1, dims[1], 5)[:, :, 1:].any()
        if dims[0] > 1:
            assert und[:, f_c2c:].reshape(len(levels), -1, dims[1], 4)[:, :, 1:].any()


@pytest.mark.parametrize("name,mask", SOFT, ids=[H.soft_tag(n, m) for n, m in SOFT])
def test_labels_of_soft_records(oracle, name, mask):
    """byte L on a soft obstacle, beside decided and undecided bytes: the soft levels, and the jumps of the level that ignores every point"""
    p, h, dims, rec = H.soft_instance(oracle, name, mask)
    w = _wrapper(p)
    levels = H.soft_levels(name, rec, mask)
    recs = [_decisions(w, r) for r, _ in levels.values()]
    L = dims[5]
    assert all((r == L).any() for r in recs)
    recs += _neighbours((dims[0], dims[1], dims[4]), L, recs[0])
    st, canon = _check_labels(p, np.stack(recs), H.soft_tag(name, mask))
    assert (st[:len(levels)] == 0).all()
    assert all((canon[k] == L).sum() == (recs[k] == L).sum() for k in range(len(levels)))   # the ignored points stay ignored, and no other point is


def test_a_mixed_batch(oracle):
    """refused, infeasible and partial records side by side: a refused entry never reaches the device and its neighbours keep their rows"""
    name = "c2n6e2pent"
    p, h, dims, rec = H.node_instance(oracle, name)
    Cn, N, R, E, O, L = dims
    w = _wrapper(p)
    levels = H.relax_levels(rec, 11)
    full = _decisions(w, levels["complete"][0])
    f_c2c = Cn * N * 6 + Cn * O * N * 5
    batch = [full.copy()]
    refused = full.copy(); refused[1] = 127
    batch.append(refused)
    flips = []
    for g in range(4):   # step 1, where the initial state pins the positions: the pair's group g decided for every other alternative
        for a in range(4):
            if a != full[f_c2c + 4 + g]:
                r = full.copy(); r[f_c2c + 4 + g] = a
                flips.append(r)
    batch += flips
    batch += [_decisions(w, levels[lv][0]) for lv in ("regions_only", "third", "only_c2c", "only_obs_front")]
    und = full.copy(); und[1] = -1   # an undecided region byte at step 1
    batch.append(und)
    batch.append(refused.copy())
    st, canon = _check_labels(p, np.stack(batch), "mixed")
    assert st[0] == 0 and st[1] == 2 and st[-1] == 2
    assert (st[2:2 + len(flips)] == 1).any(), list(st)   # (a condition on the inputs: some flip is infeasible)
    assert (st[2 + len(flips):-2] == 0).all()
    assert (canon[-2] == -1).all()   # the points of that step have no region to be taken in: no labels, whatever the verdict


# ------------------------------------------------------------------------------------------------------------------------------ b.
def _explored(name, cap, passes, max_rel):
    """a fresh solve and exploreSolutionPool(passes, max_rel, distinct=True) behind it: the pool as found, the call's answer and timing, the pool it leaves"""
    key = (name, cap, passes, max_rel)
    if key not in _EXPLORED:
        s = _fresh(name, cap)
        w = s["w"]
        rc, added = w.exploreSolutionPool(passes, max_rel, distinct=True)
        t = _timing(w)
        n = w.solutionPoolCount()
        _EXPLORED[key] = dict(w=w, solved=s, rc=rc, added=added, timing=t, err=w.lastError(), n=n, found=w.solutionPoolFound(),
                              dec=[w.solutionPoolFoundDecisions(k) for k in range(n)])
        print("DISTINCT %s capacity %d passes %d max_rel %g: %d entries, rc %d, passes run %d, nodes %d, iterations %d, still adding %d, device %.1f ms of %.1f ms"
              % (name, cap, passes, max_rel, s["n"], rc, t[2], t[3], t[4], t[5], 1e3 * t[1], 1e3 * t[0]))
    return _EXPLORED[key]


def _canonical_signatures(w, dims, recs, st):
    """per record of the last solveDecisions call of w: the signature under the filter of its host-built canonical record - of its own bytes where
    it is not feasible"""
    Cn, N, O = dims
    out = []
    for k in range(len(recs)):
        lab = _host_labels(w, k, recs.shape[1]) if st[k] == 0 else None
        out.append(P.pool_signature(Cn, N, O, FILTER, lab if lab is not None else recs[k]).tobytes())
    return out


def _replay_distinct(name, cap, max_rel):
    """the call as a host loop over pool_jumps, solveDecisions, fixedBatchRecord and poolSignature, up to 4 passes: the state behind every pass that
    ran (0: behind pass 0, the kept entries' own solves)"""
    if (name, cap, max_rel) in _REPLAY:
        return _REPLAY[(name, cap, max_rel)]
    s = _solved(name, cap)
    Cn, N, O = s["dims"]
    w = _wrapper(_params(name))
    dec, found = [d.copy() for d in s["dec"]], [float(x) for x in s["found"]]
    sigs = [P.pool_signature(Cn, N, O, FILTER, d).tobytes() for d in dec]
    if len(dec) >= cap:
        _REPLAY[(name, cap, max_rel)] = {0: dict(added=[], dec=list(dec), found=list(found), passes=0, neighbours=0, iterations=0, last=0)}
        return _REPLAY[(name, cap, max_rel)]
    own = np.stack(dec)
    rc, st, obj, viol, it, route, best = w.solveDecisions(own)
    assert rc == 0 and not (st == 2).any()
    csigs = _canonical_signatures(w, s["dims"], own, st)
    added, expand = [], list(range(len(dec)))
    neighbours, iterations = len(dec), int(it.sum())
    states = {0: dict(added=[], dec=list(dec), found=list(found), passes=0, neighbours=neighbours, iterations=iterations, last=0)}
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
        assert rc == 0 and not (st == 2).any(), (name, p)
        neighbours += total; iterations += int(it.sum())
        new, aliases = [], 0
        for g in sorted((g for g in range(total) if st[g] == 0), key=lambda g: (obj[g], g)):
            if len(dec) >= cap:
                break
            sg = P.pool_signature(Cn, N, O, FILTER, recs[g]).tobytes()
            if not _within(found[0], obj[g], max_rel) or sg in sigs:
                continue
            cs = P.pool_signature(Cn, N, O, FILTER, _host_labels(w, g, recs.shape[1])).tobytes()
            if cs in csigs:
                aliases += 1
                continue
            k, first, stride, count, value = origin[g]
            new.append(len(dec))
            added.append({"parent": k, "pass": p, "first": first, "stride": stride, "count": count, "value": value, "iterations": int(it[g]), "objective": float(obj[g])})
            dec.append(recs[g].copy()); found.append(float(obj[g])); sigs.append(sg); csigs.append(cs)
        print("REPLAY-DISTINCT %s capacity %d max_rel %g pass %d: %d expanded, %d neighbours, %d feasible, %d aliases dropped, %d admitted"
              % (name, cap, max_rel, p, len(expand), total, int((st == 0).sum()), aliases, len(new)))
        states[p] = dict(added=list(added), dec=list(dec), found=list(found), passes=p, neighbours=neighbours, iterations=iterations, last=len(new))
        if not new:
            break
        expand = new
    _REPLAY[(name, cap, max_rel)] = states
    return states


@pytest.mark.parametrize("max_rel", MAX_REL)
@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_distinct_explore_is_its_host_replay(name, cap, passes, max_rel):
    states = _replay_distinct(name, cap, max_rel)
    c = _explored(name, cap, passes, max_rel)
    s = c["solved"]
    e = states[min(passes, max(states))]
    assert c["rc"] == len(e["added"]) == len(c["added"]) and c["n"] == len(e["dec"]) == s["n"] + c["rc"], (c["rc"], len(e["added"]), c["err"])
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


# ------------------------------------------------------------------------------------------------------------------------------ c.
@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_properties(name, cap):
    """the signatures of the pool are pairwise distinct; the canonical signature of every added entry differs from that of every entry in front of
    it, so the canonical ones are pairwise distinct wherever those of the entries as found are (the full pool of cfg4 seed 9 holds aliases as found,
    which no explore removes); every added objective respects the cap; every added entry is what solveDecisions answers for its bytes, and its bytes
    are its parent's behind its jump"""
    Cn, N, O = _solved(name, cap)["dims"]
    w2 = _wrapper(_params(name))
    for max_rel in MAX_REL:
        c = _explored(name, cap, 4, max_rel)
        s = c["solved"]
        sigs = [P.pool_signature(Cn, N, O, FILTER, d).tobytes() for d in c["dec"]]
        assert len(set(sigs)) == len(sigs) == c["n"] <= cap, (name, max_rel)
        pool = np.stack(c["dec"])
        rc, st, obj, viol, it, route, best = w2.solveDecisions(pool)
        assert rc == 0
        csigs = _canonical_signatures(w2, (Cn, N, O), pool, st)
        for q in range(s["n"], c["n"]):   # what the admission guarantees: an added entry is no alias of an entry in front of it
            assert csigs[q] not in csigs[:q], (name, max_rel, q)
        if len(set(csigs[:s["n"]])) == s["n"]:   # the call removes nothing: kept entries that are aliases of each other (cfg4s9: 14 classes in 16) stay
            assert len(set(csigs)) == len(csigs), (name, max_rel, len(set(csigs)), len(csigs))
        else:
            print("PROPERTIES %s capacity %d: %d canonical signatures among the %d entries as found" % (name, cap, len(set(csigs[:s["n"]])), s["n"]))
        assert (st[s["n"]:] == 0).all()
        for j, a in enumerate(c["added"]):
            q = s["n"] + j
            assert _within(s["found"][0], a["objective"], max_rel), (name, max_rel, a)
            assert np.float64(a["objective"]).tobytes() == np.float64(obj[q]).tobytes() == np.float64(c["found"][q]).tobytes(), (name, j)
            assert a["iterations"] == it[q] and 1 <= a["pass"] <= 4 and 0 <= a["parent"] < q
            want = c["dec"][a["parent"]].copy()
            want[a["first"]:a["first"] + a["count"] * a["stride"]:a["stride"]] = a["value"]
            assert want.tobytes() == pool[q].tobytes(), (name, j)
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
    """the exploring wrapper's own solve was the solve of a wrapper nothing touched, and a solve BEHIND a distinct explore on the same wrapper equals a fresh one"""
    a = _solved(name, cap)
    c = _explored(name, cap, 1, -1.0)
    _same_solve(a, c["solved"], (name, cap, "the exploring wrapper's own solve"))
    w = c["w"]
    _same_solve(a, _as_found(w, w.callCplex()), (name, cap, "a solve behind a distinct explore"))
    _EXPLORED.pop((name, cap, 1, -1.0))   # (its pool is the new solve's now)


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_climb_and_refinement_behind_the_explore(name, cap):
    c = _explored(name, cap, 4, 0.5)
    _EXPLORED.pop((name, cap, 4, 0.5))   # (its pool is the climbed and refined one from here on)
    w, n = c["w"], c["n"]
    Cn, N, O = c["solved"]["dims"]
    rc, before, after, moves, status = w.improveSolutionPool(8)
    assert rc >= 0 and len(before) == n == w.solutionPoolCount(), (name, rc)
    for k in range(n):
        assert P.pool_signature(Cn, N, O, FILTER, w.solutionPoolFoundDecisions(k)).tobytes() == P.pool_signature(Cn, N, O, FILTER, c["dec"][k]).tobytes(), (name, k)
        assert after[k] <= before[k]
        if k >= c["solved"]["n"]:
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


# ------------------------------------------------------------------------------------------------------------------------------ d.
_MERGED = {}


def _merged(name, cap):
    """(found, behind the explore, left by solveSolutionPool) for the plain and for the distinct call: 4 passes, no cap, each on a fresh solve"""
    if (name, cap) not in _MERGED:
        row = []
        for distinct in (False, True):
            s = _fresh(name, cap)
            w = s["w"]
            rc, added = w.exploreSolutionPool(4, -1.0, distinct=distinct)
            assert rc >= 0, (name, distinct, rc, w.lastError())
            n = w.solutionPoolCount()
            assert n == s["n"] + rc
            st, obj, viol, it, route = w.solveSolutionPool()
            left = w.solutionPoolCount()
            assert left == len(obj) >= 1
            row.append((s["n"], n, left))
        _MERGED[(name, cap)] = row
        (a0, a1, a2), (b0, b1, b2) = row
        print("MERGED %-10s capacity %2d | plain %2d -> %2d -> %2d, merged %2d | distinct %2d -> %2d -> %2d, merged %2d" % (name, cap, a0, a1, a2, a1 - a2, b0, b1, b2, b1 - b2))
    return _MERGED[(name, cap)]


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_it_merges_no_more_than_the_plain_call(name, cap):
    """merged(mode) = entries behind the explore - entries solveSolutionPool leaves: merged(distinct) <= merged(plain), and never fewer entries left"""
    (a0, a1, a2), (b0, b1, b2) = _merged(name, cap)
    assert a0 == b0 and b1 - b2 <= a1 - a2 and b2 >= a2, (name, cap, (a0, a1, a2), (b0, b1, b2))


def test_it_does_what_it_is_for():
    """over the cases the distinct call has strictly fewer entries merged away than the plain call"""
    rows = [_merged(name, cap) for name, cap in CASES]
    plain = [a1 - a2 for (a0, a1, a2), _ in rows]; dist = [b1 - b2 for _, (b0, b1, b2) in rows]
    print("MERGED in all: plain %d, distinct %d" % (sum(plain), sum(dist)))
    assert sum(dist) < sum(plain), (plain, dist)

"""Decision records settled on the device (settleDecisions: the step, compaction and gather kernels of pool_settle.hip around the chain and
pool_label_kernel) and the explore that admits a manoeuvre by its settled labels (exploreSolutionPool(settled=True)); DESIGN.md 6j.

a. settleDecisions is the HOST ITERATION of canonicalDecisions (_host_settle): per record, canonicalDecisions on the current labels until they stay,
   at most pool_settle_passes() times - round by round over the records that still move, one canonicalDecisions call per round; it uses none of the
   new kernels.  Bit for bit in out, settled, solves, best and the solve and iteration counts of last_timing.
b. It is the refinement: on the pool as found, the settled rows are the labels solveSolutionPool ends on.  An entry that STAYS in the refined pool
   (the first of its class) has the refined entry's labels byte for byte and its answer bit for bit; an entry the refinement merges away has the
   signature of the entry it merges into - pool_same_entry merges by the signature under the filter, and two entries of one signature need not carry
   the same region and environment bytes, so nothing stronger holds for them.  The classes among the feasible entries number what the refinement leaves.
c. The iteration is exercised: the histogram of solves per record of the REFERENCE holds records with 2 solves and with >= 3.
d. The settled explore is its host replay (_replay_settled: test_pool_label_gpu._replay_distinct with the settled test, computed with _host_settle).
e. What it is for: L(after) == L0 + added, and over the cases the distinct call has entries merged away and the settled call none.
f. The existing calls answer as before, in front of and behind a settled call on the same wrapper.
All tests here need a real MI355X: run with  python -m pytest tests/test_pool_settle_gpu.py -m gpu -s."""
import collections
import ctypes as C

import numpy as np
import pytest

import helpers as H
import planner_miqp_amd as P
from planner_miqp_amd.ctypes_types import PoolExploreC
from test_pool_explore_gpu import CASES, FULL, IDS, MAX_REL, PASSES, _fresh, _same_solve, _solved, _timing, _within
from test_pool_filter_gpu import FILTER, _as_found, _params
from test_pool_label_gpu import ORACLE_SHAPES, SOFT, _decisions, _merged, _neighbours, _wrapper

pytestmark = pytest.mark.gpu

SETTLE_CASES = [("c2n6e2pent", 8), ("wrap", 8), ("cfg4s12", 16), ("cfg4s7", 16), ("cfg4s1", 8)]   # the first three: as the label suite; seeds 7 and 1: where one labelling is not enough
_CHECKED, _EXPLORED, _REPLAY, _L0 = {}, {}, {}, {}


def _host_settle(w, recs, first=1):
    """the reference: records whose round first - 1 is behind them (first = 1: none) solved and labelled with canonicalDecisions until the labels stay"""
    passes = P.pool_settle_passes()
    recs = np.ascontiguousarray(recs, dtype=np.int8)
    n = len(recs)
    cur = recs.copy()
    out = dict(status=np.full(n, 2, dtype=np.int32), objective=np.full(n, np.nan), violation=np.full(n, np.nan), iterations=np.zeros(n, dtype=np.int32),
               route=np.full(n, -1, dtype=np.int32))
    solves = np.zeros(n, dtype=np.int32)
    live, n_solves, n_iters, rounds = list(range(n)), 0, 0, []
    for p in range(first, passes + 1):
        if not live:
            break
        rounds.append(len(live))
        rc, st, obj, viol, it, route, best, canon = w.canonicalDecisions(cur[live])
        assert rc == 0, (rc, w.lastError())
        nxt = []
        for q, k in enumerate(live):
            for name, a in zip(("status", "objective", "violation", "iterations", "route"), (st, obj, viol, it, route)):
                out[name][k] = a[q]
            if st[q] == 2:
                continue
            solves[k] = p; n_solves += 1; n_iters += int(it[q])
            if st[q] == 0 and canon[q].tobytes() != cur[k].tobytes():
                if p < passes:
                    cur[k] = canon[q]; nxt.append(k)
                else:
                    solves[k] = -p
        live = nxt
    settled = np.where((out["status"] == 0)[:, None], cur, np.int8(-1)).astype(np.int8)
    feas = [k for k in range(n) if out["status"][k] == 0]
    best = min(feas, key=lambda k: (out["objective"][k], k)) if feas else -1
    out.update(settled=settled, solves=solves, best=best, n_solves=n_solves, n_iters=n_iters, rounds=rounds)
    return out


def _check_settle(params, recs, tag):
    """a. for one batch; returns the reference and the call's settled rows"""
    if tag in _CHECKED:
        return _CHECKED[tag]
    recs = np.ascontiguousarray(recs, dtype=np.int8)
    ref = _host_settle(_wrapper(params), recs)
    w = _wrapper(params)
    rc, st, obj, viol, it, route, best, settled, solves = w.settleDecisions(recs)
    t = _timing(w)
    hist = collections.Counter(int(x) for x in ref["solves"])
    print("SETTLE %s: %d records, live per round %s, solves per record %s, %d solves, %d iterations, device %.1f ms of %.1f ms"
          % (tag, len(recs), ref["rounds"], sorted(hist.items()), ref["n_solves"], ref["n_iters"], 1e3 * t[1], 1e3 * t[0]))
    assert rc == 0 and settled.shape == recs.shape and solves.shape == (len(recs),), (tag, rc, w.lastError())
    assert solves.tobytes() == ref["solves"].tobytes(), (tag, [(int(k), int(solves[k]), int(ref["solves"][k])) for k in np.flatnonzero(solves != ref["solves"])[:8]])
    for name, a in zip(("status", "objective", "violation", "iterations", "route"), (st, obj, viol, it, route)):
        assert a.tobytes() == ref[name].astype(a.dtype).tobytes(), (tag, name, np.flatnonzero(a != ref[name])[:8])
    assert settled.tobytes() == ref["settled"].tobytes(), (tag, np.argwhere(settled != ref["settled"])[:8])
    assert best == ref["best"], (tag, best, ref["best"])
    groups = sum(-(-m // P.fixed_batch_chunk()) for m in ref["rounds"])
    assert (t[2], t[3], t[4], t[5]) == (groups, ref["n_solves"], ref["n_iters"], 1 if (ref["solves"] < 0).any() else 0), (tag, t)
    assert ("still moved" in w.lastError()) == bool((ref["solves"] < 0).any())
    assert w.fixedBatchRecord(0)[0] == -1   # the call keeps no state for fixedBatchRecord
    _CHECKED[tag] = dict(ref=ref, settled=settled, solves=solves, status=st, objective=obj, iterations=it, route=route, hist=hist, recs=recs)
    return _CHECKED[tag]


def _pool_batch(name, cap):
    """the pool as found plus all jumps of its entries; on wrap and cfg4 seed 12 jumps of jumps until the batch is more than one chunk"""
    s = _solved(name, cap)
    recs = [d.copy() for d in s["dec"]]
    for d in s["dec"]:
        recs += _neighbours(s["dims"], s["lines"], d)
    if name in ("wrap", "cfg4s12"):
        for d in list(recs[s["n"]:]):
            if len(recs) > P.fixed_batch_chunk() + 64:
                break
            recs += _neighbours(s["dims"], s["lines"], d)
        assert len(recs) > P.fixed_batch_chunk()   # (a condition on the inputs: more than one chunk)
    return np.stack(recs)


# ------------------------------------------------------------------------------------------------------------------------------ a.
@pytest.mark.parametrize("name,cap", SETTLE_CASES, ids=["%s-%d" % c for c in SETTLE_CASES])
def test_settling_the_pool_and_its_neighbours(name, cap):
    c = _check_settle(_params(name), _pool_batch(name, cap), "%s/%d" % (name, cap))
    assert (c["status"] == 0).sum() > _solved(name, cap)["n"] and not (c["status"] == 2).any()


@pytest.mark.parametrize("name", ORACLE_SHAPES)
def test_settling_partial_records(oracle, name):
    """the relax levels of the shape's canonical complete record and the jumps of the complete one: a record with undecided bytes is labelled in
    full by its first solve and takes a second one - which, under labels that hold only within the labelling tolerance, need not be feasible: the
    record then has no settled labels, by definition"""
    p, h, dims, rec = H.node_instance(oracle, name)
    w = _wrapper(p)
    levels = H.relax_levels(rec, 11)
    recs = [_decisions(w, r) for r, _ in levels.values()]
    recs += _neighbours((dims[0], dims[1], dims[4]), dims[5], recs[0])
    c = _check_settle(p, np.stack(recs), "partial/" + name)
    assert not (c["status"] == 2).any()
    if len(levels) > 1:
        assert (np.abs(c["solves"][:len(levels)]) >= 2).any(), list(c["solves"][:len(levels)])


@pytest.mark.parametrize("name,mask", SOFT, ids=[H.soft_tag(n, m) for n, m in SOFT])
def test_settling_soft_records(oracle, name, mask):
    p, h, dims, rec = H.soft_instance(oracle, name, mask)
    w = _wrapper(p)
    levels = H.soft_levels(name, rec, mask)
    recs = [_decisions(w, r) for r, _ in levels.values()]
    L = dims[5]
    recs += _neighbours((dims[0], dims[1], dims[4]), L, recs[0])
    c = _check_settle(p, np.stack(recs), "soft/" + H.soft_tag(name, mask))
    assert not (c["status"] == 2).any()
    assert all((c["settled"][k] == L).sum() == (recs[k] == L).sum() for k in range(len(levels)) if c["status"][k] == 0)   # the ignored points stay ignored, and no other point is


def _mixed(oracle):
    name = "c2n6e2pent"
    p, h, dims, rec = H.node_instance(oracle, name)
    Cn, N, R, E, O, L = dims
    w = _wrapper(p)
    levels = H.relax_levels(rec, 11)
    full = _decisions(w, levels["complete"][0])
    f_c2c = Cn * N * 6 + Cn * O * N * 5
    refused = full.copy(); refused[1] = 127
    flips = []
    for g in range(4):
        for a in range(4):
            if a != full[f_c2c + 4 + g]:
                r = full.copy(); r[f_c2c + 4 + g] = a
                flips.append(r)
    partial = [_decisions(w, levels[lv][0]) for lv in ("regions_only", "third", "only_c2c", "only_obs_front")]
    und = full.copy(); und[1] = -1   # an undecided region byte at step 1
    return p, full, refused, flips, partial, und


def test_a_mixed_batch(oracle):
    """refused, infeasible and partial records side by side"""
    p, full, refused, flips, partial, und = _mixed(oracle)
    batch = [full.copy(), refused] + flips + partial + [und, refused.copy()]
    c = _check_settle(p, np.stack(batch), "mixed")
    st, solves = c["status"], c["solves"]
    assert st[1] == 2 and st[-1] == 2 and solves[1] == 0 and solves[-1] == 0 and (solves[st != 2] != 0).all()
    assert ((st[2:2 + len(flips)] == 1) & (solves[2:2 + len(flips)] == 1)).any(), (list(st), list(solves))   # (a condition on the inputs: some flip is infeasible at its first solve, which is its last)
    assert (c["settled"][-2] == -1).all() and (c["settled"][st != 0] == -1).all()


def _stay_and_movers():
    """of the c2n6e2pent pool batch: a record that is settled with one solve - the settled labels of a record are a fixed point - and the records
    that take more (every feasible record as found does: its step 0 bytes are the search's, the labels have -1 there)"""
    c = _check_settle(_params("c2n6e2pent"), _pool_batch("c2n6e2pent", 8), "c2n6e2pent/8")
    stay = [c["settled"][k] for k in range(len(c["recs"])) if c["solves"][k] >= 2 and c["status"][k] == 0]
    movers = [c["recs"][k] for k in range(len(c["recs"])) if abs(int(c["solves"][k])) >= 2]
    assert stay and movers   # (a condition on the inputs)
    return stay[0], movers


def test_the_scatter():
    """a batch in which only the LAST record moves, and one in which every second record moves"""
    stay, movers = _stay_and_movers()
    p = _params("c2n6e2pent")
    last = _check_settle(p, np.stack([stay] * 66 + [movers[0]]), "scatter/last")
    assert (last["solves"][:-1] == 1).all() and abs(int(last["solves"][-1])) >= 2 and last["ref"]["rounds"][:2] == [67, 1]
    second = _check_settle(p, np.stack([stay if k % 2 == 0 else movers[(k // 2) % len(movers)] for k in range(131)]), "scatter/second")
    assert (second["solves"][0::2] == 1).all() and (np.abs(second["solves"][1::2]) >= 2).all() and second["ref"]["rounds"][:2] == [131, 65]


@pytest.mark.parametrize("live", [1, 63, 64, 65, 1024, 1025])
def test_the_compaction_at(live):
    """`live` records move behind the first round, between records that do not: a wavefront, a tile of 256 and a chunk of the chain, each met exactly,
    one short and one over"""
    stay, movers = _stay_and_movers()
    batch = []
    for k in range(live):
        batch += [stay] * (k % 3) + [movers[k % len(movers)]]
    c = _check_settle(_params("c2n6e2pent"), np.stack(batch + [stay]), "compaction/%d" % live)
    assert c["ref"]["rounds"][1] == live


# ------------------------------------------------------------------------------------------------------------------------------ b.
def _refined_as_found(name, cap):
    """solveSolutionPool on a fresh solve's pool as found: its arrays, and the labels of every refined record"""
    if (name, cap) not in _L0:
        s = _fresh(name, cap)
        w = s["w"]
        st, obj, viol, it, route = w.solveSolutionPool()
        left = w.solutionPoolCount()
        assert left == len(obj) >= 1
        labels = []
        for j in range(left):
            rc, rec = w.solutionPoolRecord(j)
            labels.append(w.poolSignature(rec, 31) if rc == 0 else None)
        _L0[(name, cap)] = dict(n=s["n"], left=left, status=st, objective=obj, iterations=it, route=route, labels=labels, dec=s["dec"])
    return _L0[(name, cap)]


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_it_is_the_refinement(name, cap):
    s = _solved(name, cap)
    Cn, N, O = s["dims"]
    r = _refined_as_found(name, cap)
    assert r["n"] == s["n"] and all(a.tobytes() == b.tobytes() for a, b in zip(r["dec"], s["dec"]))
    c = _check_settle(_params(name), np.stack(s["dec"]), "found/%s/%d" % (name, cap))
    sig = [P.pool_signature(Cn, N, O, FILTER, c["settled"][k]).tobytes() if c["status"][k] == 0 else None for k in range(s["n"])]
    kept, where = [], {}
    for k in range(s["n"]):   # the refinement keeps the first entry of every class, and every entry that is not feasible
        if sig[k] is None or sig[k] not in where:
            if sig[k] is not None:
                where[sig[k]] = len(kept)
            kept.append(k)
    assert len(kept) == r["left"], (name, len(kept), r["left"])
    assert len(set(x for x in sig if x is not None)) + sum(x is None for x in sig) == r["left"]
    for j, k in enumerate(kept):
        assert (r["status"][j], r["iterations"][j], r["route"][j]) == (c["status"][k], c["iterations"][k], c["route"][k]), (name, j, k)
        assert np.float64(r["objective"][j]).tobytes() == np.float64(c["objective"][k]).tobytes(), (name, j, k)
        if sig[k] is not None:
            assert r["labels"][j].tobytes() == c["settled"][k].tobytes(), (name, j, k)
    same = 0
    for k in range(s["n"]):
        if sig[k] is not None and k not in kept:
            j = where[sig[k]]
            assert P.pool_signature(Cn, N, O, FILTER, r["labels"][j]).tobytes() == sig[k], (name, k, j)
            same += r["labels"][j].tobytes() == c["settled"][k].tobytes()
    print("REFINED %s capacity %d: %d entries as found, %d left, %d merged away of which %d carry the kept entry's labels byte for byte"
          % (name, cap, s["n"], r["left"], s["n"] - len(kept), same))


# ------------------------------------------------------------------------------------------------------------------------------ c.
def test_the_iteration_is_exercised():
    hist = collections.Counter()
    for name, cap in SETTLE_CASES:
        hist += _check_settle(_params(name), _pool_batch(name, cap), "%s/%d" % (name, cap))["hist"]
    print("SETTLE solves per record over the pool batches (reference): %s" % sorted(hist.items()))
    assert hist[2] > 0, sorted(hist.items())
    assert sum(v for k, v in hist.items() if abs(k) >= 3) > 0, sorted(hist.items())


# ------------------------------------------------------------------------------------------------------------------------------ d.
def _explored(name, cap, passes, max_rel):
    key = (name, cap, passes, max_rel)
    if key not in _EXPLORED:
        s = _fresh(name, cap)
        w = s["w"]
        rc, added = w.exploreSolutionPool(passes, max_rel, settled=True)
        t = _timing(w)
        n = w.solutionPoolCount()
        _EXPLORED[key] = dict(w=w, solved=s, rc=rc, added=added, timing=t, err=w.lastError(), n=n, found=w.solutionPoolFound(),
                              dec=[w.solutionPoolFoundDecisions(k) for k in range(n)])
        print("SETTLED %s capacity %d passes %d max_rel %g: %d entries, rc %d, passes run %d, solves %d, iterations %d, still adding %d, device %.1f ms of %.1f ms"
              % (name, cap, passes, max_rel, s["n"], rc, t[2], t[3], t[4], t[5], 1e3 * t[1], 1e3 * t[0]))
    return _EXPLORED[key]


def _replay_settled(name, cap, max_rel):
    """the call as a host loop over pool_jumps, canonicalDecisions, _host_settle and pool_signature, up to 4 passes: the state behind every pass"""
    if (name, cap, max_rel) in _REPLAY:
        return _REPLAY[(name, cap, max_rel)]
    s = _solved(name, cap)
    Cn, N, O = s["dims"]
    w = _wrapper(_params(name))
    sign = lambda d: P.pool_signature(Cn, N, O, FILTER, d).tobytes()
    dec, found = [d.copy() for d in s["dec"]], [float(x) for x in s["found"]]
    sigs = [sign(d) for d in dec]
    if len(dec) >= cap:
        _REPLAY[(name, cap, max_rel)] = {0: dict(added=[], dec=list(dec), found=list(found), passes=0, neighbours=0, iterations=0, last=0)}
        return _REPLAY[(name, cap, max_rel)]
    own = _host_settle(w, np.stack(dec))
    assert not (own["status"] == 2).any()
    ssigs = [sign(own["settled"][k]) if own["status"][k] == 0 else None for k in range(len(dec))]
    added, expand = [], list(range(len(dec)))
    neighbours, iterations = own["n_solves"], own["n_iters"]
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
        rc, st, obj, viol, it, route, best, canon = w.canonicalDecisions(recs)
        assert rc == 0 and not (st == 2).any(), (name, p)
        neighbours += total; iterations += int(it.sum())
        # the candidates: feasible, within the cap, of a signature that is new against the pool at the start of the pass
        cand = [g for g in range(total) if st[g] == 0 and _within(found[0], obj[g], max_rel) and sign(recs[g]) not in sigs]
        moved = [g for g in cand if canon[g].tobytes() != recs[g].tobytes()]
        fin = {g: (recs[g], 1) for g in cand if g not in set(moved)}   # neighbour -> (settled labels or None, solves)
        if moved:
            r = _host_settle(w, canon[moved], first=2)
            neighbours += r["n_solves"]; iterations += r["n_iters"]
            for q, g in enumerate(moved):
                fin[g] = (r["settled"][q] if r["status"][q] == 0 else None, abs(int(r["solves"][q])))
        new, slid = [], 0
        for g in sorted(cand, key=lambda g: (obj[g], g)):
            if len(dec) >= cap:
                break
            sg = sign(recs[g])
            if sg in sigs or fin[g][0] is None:
                continue
            ss = sign(fin[g][0])
            if ss in ssigs:
                slid += 1
                continue
            k, first, stride, count, value = origin[g]
            new.append(len(dec))
            added.append({"parent": k, "pass": p, "first": first, "stride": stride, "count": count, "value": value, "iterations": int(it[g]), "objective": float(obj[g]),
                          "solves": fin[g][1]})
            dec.append(recs[g].copy()); found.append(float(obj[g])); sigs.append(sg); ssigs.append(ss)
        print("REPLAY-SETTLED %s capacity %d max_rel %g pass %d: %d expanded, %d neighbours, %d feasible, %d candidates, %d entered the settle rounds, %d dropped by the settled signature, %d admitted"
              % (name, cap, max_rel, p, len(expand), total, int((st == 0).sum()), len(cand), len(moved), slid, len(new)))
        states[p] = dict(added=list(added), dec=list(dec), found=list(found), passes=p, neighbours=neighbours, iterations=iterations, last=len(new))
        if not new:
            break
        expand = new
    _REPLAY[(name, cap, max_rel)] = states
    return states


@pytest.mark.parametrize("max_rel", MAX_REL)
@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_settled_explore_is_its_host_replay(name, cap, passes, max_rel):
    states = _replay_settled(name, cap, max_rel)
    c = _explored(name, cap, passes, max_rel)
    s = c["solved"]
    e = states[min(passes, max(states))]
    assert c["rc"] == len(e["added"]) == len(c["added"]) and c["n"] == len(e["dec"]) == s["n"] + c["rc"], (c["rc"], len(e["added"]), c["err"])
    for a, b in zip(c["added"], e["added"]):
        assert {k: v for k, v in a.items() if k != "objective"} == {k: v for k, v in b.items() if k != "objective"}, (a, b)
        assert np.float64(a["objective"]).tobytes() == np.float64(b["objective"]).tobytes(), (a, b)
        assert 1 <= a["solves"] <= P.pool_settle_passes()
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


@pytest.mark.parametrize("name,cap", [CASES[0], CASES[1], CASES[3]], ids=[IDS[0], IDS[1], IDS[3]])
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
    a = _solved(name, cap)
    c = _explored(name, cap, 1, -1.0)
    _same_solve(a, c["solved"], (name, cap, "the exploring wrapper's own solve"))
    w = c["w"]
    _same_solve(a, _as_found(w, w.callCplex()), (name, cap, "a solve behind a settled explore"))
    _EXPLORED.pop((name, cap, 1, -1.0))   # (its pool is the new solve's now)


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_climb_and_refinement_behind_the_explore(name, cap):
    c = _explored(name, cap, 4, 0.5)
    _EXPLORED.pop((name, cap, 4, 0.5))   # (its pool is the climbed and refined one from here on)
    w, n = c["w"], c["n"]
    rc, before, after, moves, status = w.improveSolutionPool(8)
    assert rc >= 0 and len(before) == n == w.solutionPoolCount(), (name, rc)
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


# ------------------------------------------------------------------------------------------------------------------------------ e.
_LEFT = {}


def _left_behind_settled(name, cap):
    """(found, behind the settled explore of 4 passes without a cap, left by solveSolutionPool)"""
    if (name, cap) not in _LEFT:
        c = _explored(name, cap, 4, -1.0)
        _EXPLORED.pop((name, cap, 4, -1.0))   # (its pool is the refined one from here on)
        assert c["rc"] >= 0, (name, c["rc"], c["err"])
        st, obj, viol, it, route = c["w"].solveSolutionPool()
        left = c["w"].solutionPoolCount()
        assert left == len(obj) >= 1
        _LEFT[(name, cap)] = (c["solved"]["n"], c["n"], left)
    return _LEFT[(name, cap)]


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_the_refinement_keeps_what_the_call_added(name, cap):
    """L(after) == L0 + added: solveSolutionPool behind the settled explore merges away nothing the call added"""
    n0, n1, left = _left_behind_settled(name, cap)
    l0 = _refined_as_found(name, cap)["left"]
    print("KEPT %-10s capacity %2d | as found %2d -> %2d | settled %2d -> %2d -> %2d, added %2d" % (name, cap, n0, l0, n0, n1, left, n1 - n0))
    assert left == l0 + (n1 - n0), (name, cap, n0, l0, n1, left)


def _added_and_merged(name, cap):
    """of the entries each call ADDED, how many the refinement merges away: behind - left - (found - L0), for the distinct and for the settled call"""
    l0 = _refined_as_found(name, cap)["left"]
    (_, _, _), (b0, b1, b2) = _merged(name, cap)
    n0, n1, left = _left_behind_settled(name, cap)
    return (n0, l0), (b0, b1, b2, (b1 - b2) - (b0 - l0)), (n0, n1, left, (n1 - left) - (n0 - l0))


@pytest.mark.parametrize("name,cap", CASES, ids=IDS)
def test_against_the_distinct_call(name, cap):
    """the same quantity for the distinct call on the same case: the settled call never has more of its additions merged away"""
    (n0, l0), d, t = _added_and_merged(name, cap)
    print("ADDED-AND-MERGED %-10s capacity %2d | as found %2d -> %2d | distinct %2d -> %2d -> %2d: %2d | settled %2d -> %2d -> %2d: %2d" % ((name, cap, n0, l0) + d + t))
    assert d[0] == t[0] == n0 and 0 == t[3] <= d[3], (name, cap, d, t)


def test_it_does_what_it_is_for():
    """over the cases the distinct call has additions merged away, the settled call none"""
    rows = [_added_and_merged(name, cap) for name, cap in CASES]
    dist, sett = [d[3] for _, d, _ in rows], [t[3] for _, _, t in rows]
    print("ADDED-AND-MERGED in all: distinct %d, settled %d" % (sum(dist), sum(sett)))
    assert sum(dist) > 0, dist
    assert all(x == 0 for x in sett), sett


# ------------------------------------------------------------------------------------------------------------------------------ f.
def _raw_explore(w, fn):
    out = (PoolExploreC * P.pool_max())()
    rc = int(fn(w._h, 4, -1.0, out, P.pool_max()))
    n = w.solutionPoolCount()
    return rc, bytes(bytearray(out)[:max(rc, 0) * C.sizeof(PoolExploreC)]), [o.reserved for o in out[:max(rc, 0)]], w.solutionPoolFound().tobytes(), \
        [w.solutionPoolFoundDecisions(k).tobytes() for k in range(n)], _timing(w)[2:]


@pytest.mark.parametrize("mode,name,cap", [("plain", "c2n6e2pent", 8), ("distinct", "cfg4s12", 16)])
def test_the_existing_explores_are_untouched(mode, name, cap):
    """the call in front of and behind a settled call on the same wrapper, each behind a solve of its own: the same bytes, reserved 0"""
    s = _fresh(name, cap)
    w = s["w"]
    fn = w._L.miqp_solver_pool_explore if mode == "plain" else w._L.miqp_solver_pool_explore_distinct
    a = _raw_explore(w, fn)
    assert w.callCplex() == P.OptimizationStatus.SUCCESS
    rc, added = w.exploreSolutionPool(4, -1.0, settled=True)
    assert rc >= 0 and all("solves" in x for x in added)
    assert w.callCplex() == P.OptimizationStatus.SUCCESS
    b = _raw_explore(w, fn)
    assert a == b and a[0] > 0 and all(x == 0 for x in a[2]), (mode, name, a[0], b[0])
    if mode == "distinct":   # (the dicts of the two existing modes keep their keys)
        rc, added = w.exploreSolutionPool(4, -1.0, distinct=True) if w.callCplex() == P.OptimizationStatus.SUCCESS else (-9, [])
        assert rc == a[0] and all(set(x) == {"parent", "pass", "first", "stride", "count", "value", "iterations", "objective"} for x in added)


def test_canonical_decisions_are_untouched():
    name, cap = "wrap", 8
    s = _solved(name, cap)
    recs = np.stack([d.copy() for d in s["dec"]] + [r for d in s["dec"] for r in _neighbours(s["dims"], s["lines"], d)])
    w = _wrapper(_params(name))
    a = w.canonicalDecisions(recs)
    assert w.settleDecisions(recs)[0] == 0
    b = w.canonicalDecisions(recs)
    assert a[0] == b[0] == 0 and a[6] == b[6] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:6] + a[7:], b[1:6] + b[7:]))
    assert w.fixedBatchRecord(int(a[6]))[0] == 0   # (canonicalDecisions keeps its state for fixedBatchRecord, as before)

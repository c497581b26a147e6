"""solveFixedBatch - many fix records of one instance as nodes of common launches - against the oracle and against solveFixed, entry by entry.

The chain of node kernels hands nodes on between its launches (ovf_list to the larger on-chip block, ovf2_list to the memory-backed kernel);
test_node_qp_gpu.py pins it with one node per launch.  Here the levels of a shape go through it TOGETHER, so nodes of different size share a
launch, and each entry is held against the oracle's solve_fixed (the tolerances of test_node_qp_gpu.py: the same pair of solvers at the same QP
tolerance) and, bit for bit, against what solveFixed returns for that record alone.  The oracle's answers are those of test_node_qp_gpu.py
(computed once per session).  All tests here need a real MI355X: run with  python -m pytest tests/test_fixed_batch_gpu.py -m gpu."""
import numpy as np
import pytest

import helpers as H
import planner_miqp_amd as P
from test_node_qp_gpu import LEAF_FIELDS, OBJ_RTOL, RAW_TOL, STATE_TOL, _assert_matches_oracle, _bytes, _case

pytestmark = pytest.mark.gpu

SHAPES = ["c2n6e2pent", "c2n20a", "c1n6r16hex", "mini3"]
ROUTES_MIXED = {"c2n6e2pent": {0, 1}, "c2n20a": {1, 2}, "c1n6r16hex": {0}, "mini3": {3}}
INFEASIBLE_SHAPES = sorted({e[0] for e in H.INFEASIBLE_NODES})
_WRAPPERS, _BATCH = {}, {}


def _wrapper(oracle, name):
    if name not in _WRAPPERS:
        w = P.CplexWrapper(); w.resetParameters(H.node_instance(oracle, name)[0])
        _WRAPPERS[name] = w
    return _WRAPPERS[name]


def _run(w, records):
    """one batch call: the five arrays, best, and the record of every feasible entry (fetched at once: the next parameters drop them)"""
    st, obj, viol, it, route, best = w.solveFixedBatch(records)
    recs = []
    for k in range(len(records)):
        rc, r = w.fixedBatchRecord(k)
        assert rc == (0 if st[k] == 0 else 1), (k, rc, st[k])
        recs.append(r)
    return dict(status=st, objective=obj, violation=viol, iterations=it, route=route, best=best, records=recs)


def _entry_bytes(b, k):
    """everything the call says about entry k, as bytes"""
    head = b"".join(np.asarray(b[n][k]).tobytes() for n in ("status", "route", "iterations", "objective", "violation"))
    return head + (_bytes(b["records"][k], b["objective"][k]) if b["records"][k] is not None else b"")


def _all_levels(oracle, name):
    if name not in _BATCH:
        levels = H.level_names(H.shape_dims(name))
        records = [_case(oracle, name, lv)[0] for lv in levels]
        _BATCH[name] = (levels, records, _run(_wrapper(oracle, name), records))
    return _BATCH[name]


def _single(w, record):
    rc, out, obj, it = w.solveFixed(record)
    return rc, out, obj, it, w.lastFixedRoute()


@pytest.mark.parametrize("name", SHAPES)
def test_batch_matches_the_oracle_with_routes_mixed_in_one_launch(oracle, name):
    """every level of the shape in ONE call: the oracle's verdict, objective within 1e-7 relative, continuous fields within 1e-5, every asserted
    binary kept, the complete level feasible for the raw big-M model - and the launches that solved the entries are those the shape is here for"""
    levels, records, b = _all_levels(oracle, name)
    h = H.node_instance(oracle, name)[1]
    print("FIXEDBATCH %s routes %s iterations %s best %d" % (name, list(b["route"]), list(b["iterations"]), b["best"]))
    for k, lv in enumerate(levels):
        record, ost, ores, oobj = _case(oracle, name, lv)
        assert ost == 0
        assert b["status"][k] == 0 and b["violation"][k] <= 1e-6, (name, lv, b["status"][k], b["violation"][k])
        out, obj = b["records"][k], float(b["objective"][k])
        _assert_matches_oracle("%s/%s in a batch" % (name, lv), int(b["status"][k]), out, obj, ost, ores, oobj)
        assert np.array_equal(out.active_region[:, 1:], record.active_region[:, 1:])
        for n in LEAF_FIELDS:
            assert np.all(getattr(out, n)[:, :, 1:][getattr(record, n)[:, :, 1:] == 0] == 0), (name, lv, n)
        if lv == "complete":
            v, robj, worst = oracle.raw_eval(h, out)
            print("FIXEDBATCH %s/%s raw-model violation %.2e (%s)" % (name, lv, v, worst))
            assert v < RAW_TOL and abs(robj - obj) <= 1e-6 * max(1.0, abs(obj)), (name, worst, robj, obj)
    assert set(int(r) for r in b["route"]) == ROUTES_MIXED[name], (name, list(b["route"]))
    feas = [k for k in range(len(levels)) if b["status"][k] == 0]
    assert b["best"] == min(feas, key=lambda k: (b["objective"][k], k))


@pytest.mark.parametrize("name", SHAPES)
def test_batch_equals_the_single_call_bit_for_bit(oracle, name):
    """status, route, iterations, the bytes of the objective and of every field of the record: what solveFixed + lastFixedRoute give for the
    record alone on the same wrapper.

    mini3 is here for the wide memory-backed kernel (two wavefronts per node): its stage loop adds the rows' contributions with LDS atomics,
    and the order between the wavefronts has to be fixed for a node to give the same bits alone and among others."""
    levels, records, b = _all_levels(oracle, name)
    w = _wrapper(oracle, name)
    for k, lv in enumerate(levels):
        rc, out, obj, it, route = _single(w, records[k])
        assert (rc, route, it) == (int(b["status"][k]), int(b["route"][k]), int(b["iterations"][k])), (name, lv, rc, route, it, b["status"][k], b["route"][k], b["iterations"][k])
        assert np.float64(obj).tobytes() == np.float64(b["objective"][k]).tobytes(), (name, lv, obj, b["objective"][k])
        assert _bytes(out, obj) == _bytes(b["records"][k], b["objective"][k]), (name, lv)


@pytest.mark.parametrize("name", INFEASIBLE_SHAPES)
def test_infeasible_and_refused_entries_among_feasible_ones(oracle, name):
    """[feasible, infeasible, the same feasible, a record of another shape, the same feasible]: statuses 0, 1, 0, 2, 0; the three feasible
    entries are byte-equal to each other and to the single call, best is the first of them; reversed, the batch gives the reversed results"""
    _, cls, key, alt = next(e for e in H.INFEASIBLE_NODES if e[0] == name)
    p, h, dims, rec = H.node_instance(oracle, name)
    bad = H.infeasible_record(rec, cls, key, alt)
    assert oracle.solve_fixed(h, dims, bad)[0] == 1
    good = _case(oracle, name, "third")[0]
    other = H.node_instance(oracle, "c1n2r16")[3]
    batch = [good, bad, good, other, good]
    w = _wrapper(oracle, name)
    b = _run(w, batch)
    assert list(b["status"]) == [0, 1, 0, 2, 0], list(b["status"])
    assert b["route"][3] == -1 and np.isnan(b["objective"][3])
    assert _entry_bytes(b, 0) == _entry_bytes(b, 2) == _entry_bytes(b, 4)
    assert b["best"] == 0
    r = _run(w, batch[::-1])
    assert r["best"] == 0
    for k in range(5):
        assert _entry_bytes(r, 4 - k) == _entry_bytes(b, k), k
    rc, out, obj, it, route = _single(w, good)
    assert (rc, route, it) == (0, int(b["route"][0]), int(b["iterations"][0]))
    assert _bytes(out, obj) == _bytes(b["records"][0], b["objective"][0])
    rc, out, obj, it, route = _single(w, bad)
    assert (rc, route, it) == (1, int(b["route"][1]), int(b["iterations"][1])) and np.float64(obj).tobytes() == np.float64(b["objective"][1]).tobytes()


def _c1n2r16_records(oracle):
    """c1n2r16 has no leaf disjunctions, hence ONE level, and its records differ in the region of step 1 alone: of its possible regions (0, 1, 14, 15)
    only the level's own, 15, is feasible for the oracle.  The infeasible record is the level with region 1 at step 1 (H.INFEASIBLE_NODES has no
    entry of this shape, and a record of another shape would be refused, not infeasible)."""
    p, h, dims, rec = H.node_instance(oracle, "c1n2r16")
    bad = H.copy_record(rec); bad.active_region[0, 1, :] = 0; bad.active_region[0, 1, 1] = 1
    cycle = [_case(oracle, "c1n2r16", lv)[0] for lv in H.level_names(dims)]
    assert all(oracle.solve_fixed(h, dims, r)[0] == 0 for r in cycle) and oracle.solve_fixed(h, dims, bad)[0] == 1
    return cycle, bad


def test_chunk_boundary(oracle):
    """chunk + 3 entries of the smallest shape, the infeasible record on either side of the boundary: entry k equals entry k mod L, the two
    infeasible ones are status 1, best is the lowest index among the entries with the minimum objective"""
    chunk = P.fixed_batch_chunk()
    cycle, bad = _c1n2r16_records(oracle)
    L, n = len(cycle), chunk + 3
    batch = [cycle[k % L] for k in range(n)]
    batch[chunk - 1] = bad; batch[chunk] = bad
    b = _run(_wrapper(oracle, "c1n2r16"), batch)
    assert b["status"][chunk - 1] == 1 and b["status"][chunk] == 1
    base = [_entry_bytes(b, k) for k in range(L)]
    assert all(b["status"][k] == 0 for k in range(L))
    for k in range(n):
        if k not in (chunk - 1, chunk):
            assert _entry_bytes(b, k) == base[k % L], k
    feas = [k for k in range(n) if b["status"][k] == 0]
    lowest = min(b["objective"][k] for k in feas)
    assert b["best"] == min(k for k in feas if b["objective"][k] == lowest) == 0
    rc, out, obj, it, route = _single(_wrapper(oracle, "c1n2r16"), cycle[0])
    assert rc == 0 and _bytes(out, obj) == _bytes(b["records"][0], b["objective"][0])


def test_best_is_the_first_minimum_within_a_lane_across_lanes_and_across_chunks(oracle):
    """The minimum of a handle is reduced by ONE wavefront per segment of a chunk (fixed_collect_kernel of csrc/fixed_chain.hip): lane k mod 64 walks
    nodes k, k + 64, ..., an xor tree joins the lanes, the host folds the chunks.  Two feasible records of `mini` - A, the complete level, and B, regions
    only, which the oracle answers with a lower objective - with B at 70, 71 and 134 of 140 entries: 70 and 134 meet in one lane, 70 and 71 in
    neighbouring ones, and best is 70.  The same list as handle 1 of a two-handle call, behind a handle of 3 records, gives the same best; and with B
    only at 1025 of 1030 entries the minimum lies in the second launch group."""
    (a, rca, _, obja), (b, rcb, _, objb) = _case(oracle, "mini", "complete"), _case(oracle, "mini", "regions_only")
    assert rca == rcb == 0 and obja > objb + 1.0, (rca, rcb, obja, objb)
    p = H.node_instance(oracle, "mini")[0]
    batch = [a] * 140
    for k in (70, 71, 134):
        batch[k] = b
    r = _run(_wrapper(oracle, "mini"), batch)
    print("FIXEDBATCH best-in-lanes objectives A %r B %r best %d" % (float(r["objective"][0]), float(r["objective"][70]), r["best"]))
    assert all(s == 0 for s in r["status"]) and r["objective"][70] < r["objective"][0]
    assert r["best"] == 70
    assert _entry_bytes(r, 70) == _entry_bytes(r, 71) == _entry_bytes(r, 134)
    ws = []
    for _ in range(2):
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    multi = P.solve_fixed_multi(ws, [[a, a, a], batch])
    assert multi[0][5] == 0 and multi[1][5] == 70, (multi[0][5], multi[1][5])
    assert multi[1][1].tobytes() == r["objective"].tobytes()
    chunk = P.fixed_batch_chunk()
    assert chunk == 1024
    big = [a] * 1030; big[1025] = b
    st, obj, viol, it, route, best = _wrapper(oracle, "mini").solveFixedBatch(big)
    assert all(s == 0 for s in st) and best == 1025, best


def test_the_same_batch_twice_gives_the_same_bytes(oracle):
    """... in all five arrays, in best and in the records, with a solveFixed call in between"""
    levels, records, first = _all_levels(oracle, "c2n20a")
    w = _wrapper(oracle, "c2n20a")
    second = _run(w, records)
    _single(w, records[0])
    third = _run(w, records)
    for other in (second, third):
        for n in ("status", "objective", "violation", "iterations", "route"):
            assert first[n].tobytes() == other[n].tobytes(), n
        assert first["best"] == other["best"]
        assert all(_entry_bytes(first, k) == _entry_bytes(other, k) for k in range(len(records)))


def test_a_batch_call_leaves_the_solve_alone(oracle):
    """solve() on the same wrapper returns, after a batch call, the status and the objective it returned before, bit for bit"""
    from planner_miqp_amd import synthetic
    w = P.CplexWrapper(); w.resetParameters(synthetic.generate("mini", 0))
    st1 = w.callCplex(); obj1 = w.getSolutionProperties().objective
    records = [_case(oracle, "mini", lv)[0] for lv in H.level_names(H.shape_dims("mini"))] + [w.getRawResults()]   # (records of the shape; what they decide does not matter here)
    b = _run(w, records)
    assert all(s in (0, 1) for s in b["status"])
    st2 = w.callCplex(); obj2 = w.getSolutionProperties().objective
    assert st1 == st2 == P.OptimizationStatus.SUCCESS
    assert np.float64(obj1).tobytes() == np.float64(obj2).tobytes(), (obj1, obj2)

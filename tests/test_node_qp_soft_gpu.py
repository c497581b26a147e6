"""Soft obstacles node by node: the device's solveFixed, solveFixedBatch and solve_fixed_multi against the oracle's solve_fixed on fix records
that IGNORE points of a soft obstacle.

An ignored point is the byte L (the obstacle's edge count) in a fix record.  Whoever reads the record must emit no row for the point and add
WEIGHTS_SLACK_OBSTACLE to the objective: the shared on-chip decode, the memory-backed kernel in both its widths, and the host code that turns a
RawResults record into the byte (fix_from_results) and charges the price.  Every whole-solve test of soft obstacles can close on the same optimum
with one of them wrong; here each case is ONE continuous QP - the canonical complete record of a node shape on the same instance with one
obstacle made soft (helpers.SOFT_CASES: WEIGHTS_SLACK_OBSTACLE = 0.37, a per-obstacle mask) and a chosen set of its points ignored
(helpers.SOFT_LEVELS) - and the oracle solves the same QP with the same precedence.  test_node_records_cpu.py checks the reference side without a
device: the oracle's objective is the raw big-M statement's, and the ignored rows BIND on a one-car on-chip shape, on cfg4's shape, beyond the on-chip
kernels and on the wide kernel (drop, the hard complete objective minus the soft one net of the price, as measured there: c1n2r32o 1.146,
c1n6r16hex 5.946 / 5.559 on soft_all / soft_front, c2n20a mask 0100 26.22 / 15.72 on soft_all / soft_odd_steps, c1n21o 25.65, c3n6o 0.3156; on
c2n6e2pent, c2n20b and c2n20a mask 1000 the soft obstacle's rows are slack and the cases pin the price and the decode of the byte alone).

What these tests found: every kernel skips the rows of a byte L (all four launches, with the states within 1e-5 of the oracle's on the levels whose
rows bind), and NO fixed-record entry charged the price - miqp_solver_solve_fixed added the constant of step 0 alone, and so did the collect kernels of
solveFixedBatch and solve_fixed_multi, which the pool calls share: objectives short by 0.37 per ignored point.  Fixed in miqp_solver_solve_fixed and in
soft_cost of csrc/fixed_chain.hip.  Routes found on the device: 0 on c1n2r32o and c1n6r16hex, 1 on c2n6e2pent, 2 on c2n20a and c2n20b, 3 on c1n21o and
c3n6o, on every level of each.

The raw big-M model is asked in full (violation < 1e-5, raw objective within 1e-6 of the returned one) on the five levels that decide every
disjunction, and on soft_third_undecided of the one-car shapes, which have no car/car disjunction.  With two and three cars that level leaves
car/car disjunctions undecided, and a record completed from a relaxation is no point of the raw model: where no side of an undecided car/car
disjunction holds the device reports the slack that side would need, beyond maximum_slack (A8.slack_ub violated by 7.7 on c2n6e2pent, by 12 to 22 on
cfg4's shape, by 15 on c3n6o), and the oracle's own record costs the raw model more than the node on cfg4's shape (test_node_records_cpu.py).  There
the test asserts that the raw objective is not below the returned one.  All tests here need a real MI355X: run with  python -m pytest tests/test_node_qp_soft_gpu.py -m gpu."""
import numpy as np
import pytest

import helpers as H
import planner_miqp_amd as P
from test_node_qp_gpu import LEAF_FIELDS, RAW_TOL, _assert_matches_oracle, _bytes
from test_node_qp_gpu import _case as _hard_case

pytestmark = pytest.mark.gpu

CASES = [(name, mask, level) for name, mask in H.SOFT_CASES for level in H.SOFT_LEVELS]
_IDS = ["%s-%s" % (H.soft_tag(n, m), lv) for n, m, lv in CASES]
_PAIR_IDS = [H.soft_tag(n, m) for n, m in H.SOFT_CASES]

# Which launch solved each case (the numbering of test_node_qp_gpu.EXPECTED_ROUTE), found on the device: the one-car on-chip shapes on the standard
# block (0), every level of c2n6e2pent on the larger block (1: as its complete level), every level of cfg4's shape on the memory-backed kernel behind
# them (2: one soft obstacle of four, even wholly ignored, leaves more general rows than the larger block holds), c1n21o and c3n6o on the memory-backed
# kernel of shapes without an on-chip stage (3: narrow and two wavefronts per node).
_ROUTE_OF_SHAPE = {"c1n2r32o": 0, "c1n6r16hex": 0, "c2n6e2pent": 1, "c2n20a": 2, "c2n20b": 2, "c1n21o": 3, "c3n6o": 3}
EXPECTED_ROUTE = {(name, mask, level): _ROUTE_OF_SHAPE[name] for name, mask, level in CASES}

_WRAPPERS, _ORACLE, _ROUTES = {}, {}, {}


def _wrapper(oracle, name, mask):
    if (name, mask) not in _WRAPPERS:
        w = P.CplexWrapper(); w.resetParameters(H.soft_instance(oracle, name, mask)[0])
        _WRAPPERS[(name, mask)] = w
    return _WRAPPERS[(name, mask)]


def _case(oracle, name, mask, level):
    """(record, ignored points, oracle's rc, result, objective) of one case; computed once and left unchanged"""
    if (name, mask, level) not in _ORACLE:
        p, h, dims, rec = H.soft_instance(oracle, name, mask)
        for lv, (r, pts) in H.soft_levels(name, rec, mask).items():
            _ORACLE[(name, mask, lv)] = (r, pts) + tuple(oracle.solve_fixed(h, dims, r)[:3])
    return _ORACLE[(name, mask, level)]


def _single(w, record):
    rc, out, obj, it = w.solveFixed(record)
    return rc, out, obj, it, w.lastFixedRoute()


def _soft_bytes(out, obj):
    """_bytes and the two slack fields, which it leaves out"""
    return _bytes(out, obj) + b"".join(np.ascontiguousarray(getattr(out, n)).tobytes() for n in ("slackvarsObstacle", "slackvarsObstacle_front"))


def _assert_points(tag, out, pts):
    assert H.ignored_points(out) == pts, (tag, len(H.ignored_points(out)), len(pts))
    for c, o, i, pt in pts:
        assert np.all((out.deltacc[c, o, i] if pt == 0 else out.deltacc_front[c, o, i, :, pt - 1]) == 1), (tag, c, o, i, pt)


@pytest.mark.parametrize("name,mask,level", CASES, ids=_IDS)
def test_soft_node_matches_the_oracle(oracle, name, mask, level):
    """same verdict; objective within 1e-7 relative - it carries 0.37 per ignored point - and every continuous field within 1e-5 of the oracle's; the
    returned record has slackvarsObstacle* == 1 exactly at the ignored points and every deltacc entry 1 there; asserted regions and leaf zeros are
    kept; the record is feasible for the raw big-M model and its raw objective is the returned one within 1e-6 relative (soft_third_undecided with two
    and three cars: the raw objective is not below it, and the violation is not asked); the launch that solved the node is the recorded one"""
    record, pts, ost, ores, oobj = _case(oracle, name, mask, level)
    tag = "%s/%s" % (H.soft_tag(name, mask), level)
    rc, out, obj, it, route = _single(_wrapper(oracle, name, mask), record)
    _ROUTES[(name, mask, level)] = route
    print("NODEQPSOFT %s rc %d route %d points %d" % (tag, rc, route, len(pts)))
    assert ost == 0   # (test_node_records_cpu.py: every soft level is feasible for the oracle)
    _assert_matches_oracle(tag, rc, out, obj, ost, ores, oobj)
    _assert_points(tag, out, pts)
    assert np.array_equal(out.active_region[:, 1:], record.active_region[:, 1:])
    for n in LEAF_FIELDS:
        assert np.all(getattr(out, n)[:, :, 1:][getattr(record, n)[:, :, 1:] == 0] == 0), (tag, n)
    v, robj, worst = oracle.raw_eval(H.soft_instance(oracle, name, mask)[1], out)
    print("NODEQPSOFT %s raw-model violation %.2e (%s) raw objective %.10f returned %.10f" % (tag, v, worst, robj, obj))
    if level != "soft_third_undecided" or H.shape_dims(name)[0] == 1:
        assert v < RAW_TOL and abs(robj - obj) <= 1e-6 * max(1.0, abs(obj)), (tag, worst, v, robj, obj)
    else:   # (undecided car/car disjunctions: the completed record is no point of the raw model - the module docstring - and costs it no less than the node)
        assert robj >= obj - 1e-6 * max(1.0, abs(obj)), (tag, robj, obj)
    assert route == EXPECTED_ROUTE[(name, mask, level)], (tag, route)


def test_every_route_solves_a_record_with_a_byte_L(oracle):
    """each launch of the chain - standard on-chip block, larger block, memory-backed kernel behind them, memory-backed kernel of a shape without
    an on-chip stage - solves at least one soft case, and every soft case ignores at least one point"""
    for name, mask, level in CASES:
        if (name, mask, level) not in _ROUTES:   # (the cases were not run in this session: only their routes are needed)
            _ROUTES[(name, mask, level)] = _single(_wrapper(oracle, name, mask), _case(oracle, name, mask, level)[0])[4]
        assert len(_case(oracle, name, mask, level)[1]) > 0
    count = {r: sum(1 for v in _ROUTES.values() if v == r) for r in (0, 1, 2, 3)}
    print("NODEQPSOFT cases per route", count)
    assert all(count[r] >= 1 for r in (0, 1, 2, 3)), count
    assert set(_ROUTES) == set(CASES) and all(v in (0, 1, 2, 3) for v in _ROUTES.values())
    assert {r for r in (0, 1, 2, 3)} == {EXPECTED_ROUTE[c] for c in CASES}


# ---------------------------------------------------------------------------------------------------------------- batches
def _take(w, res):
    st, obj, viol, it, route, best = res
    recs = []
    for k in range(len(st)):
        rc, r = w.fixedBatchRecord(k)
        assert rc == (0 if st[k] == 0 else 1), (k, rc, st[k])
        recs.append(r)
    return dict(status=st, objective=obj, violation=viol, iterations=it, route=route, best=best, records=recs)


def _assert_entry_is_the_single_call(tag, b, k, single):
    rc, out, obj, it, route = single
    assert (rc, route, it) == (int(b["status"][k]), int(b["route"][k]), int(b["iterations"][k])), (tag, rc, route, it, b["status"][k], b["route"][k], b["iterations"][k])
    assert np.float64(obj).tobytes() == np.float64(b["objective"][k]).tobytes(), (tag, obj, b["objective"][k])
    assert _soft_bytes(out, obj) == _soft_bytes(b["records"][k], b["objective"][k]), tag


@pytest.mark.parametrize("name,mask", H.SOFT_CASES, ids=_PAIR_IDS)
def test_soft_levels_in_one_batch_equal_the_single_calls_bit_for_bit(oracle, name, mask):
    """all soft levels of a shape in ONE solveFixedBatch call: status, route, iterations, the bytes of the objective and of every field of the record
    are those of solveFixed for the record alone - the price of the ignored points is added on the device there and on the host here"""
    w = _wrapper(oracle, name, mask)
    records = [_case(oracle, name, mask, lv)[0] for lv in H.SOFT_LEVELS]
    b = _take(w, w.solveFixedBatch(records))
    print("NODEQPSOFT batch %s routes %s objectives %s" % (H.soft_tag(name, mask), list(b["route"]), ["%.6f" % o for o in b["objective"]]))
    for k, lv in enumerate(H.SOFT_LEVELS):
        assert b["status"][k] == 0
        _assert_entry_is_the_single_call("%s/%s" % (H.soft_tag(name, mask), lv), b, k, _single(w, records[k]))
        oobj = _case(oracle, name, mask, lv)[4]
        assert abs(b["objective"][k] - oobj) <= 1e-7 * max(1.0, abs(oobj)), (name, lv, b["objective"][k], oobj)
    feas = list(range(len(records)))
    assert b["best"] == min(feas, key=lambda k: (b["objective"][k], k))


def test_a_soft_handle_beside_others_of_its_shape_in_one_multi_call(oracle):
    """c2n20a with obstacle 1 soft, with obstacle 0 soft and all hard - three handles of one shape that differ in the soft flags alone - in ONE
    solve_fixed_multi call, the soft handles with their soft levels, the hard one with its hard levels: every entry is what solveFixed says about
    the record on a twin wrapper of its handle, byte for byte (the weight and the price are taken per node from the node's instance)"""
    masks = [(0, 1, 0, 0), (1, 0, 0, 0)]
    ps = [H.soft_instance(oracle, "c2n20a", m)[0] for m in masks] + [H.node_instance(oracle, "c2n20a")[0]]
    lists = [[_case(oracle, "c2n20a", m, lv)[0] for lv in H.SOFT_LEVELS] for m in masks]
    lists.append([_hard_case(oracle, "c2n20a", lv)[0] for lv in H.level_names(H.shape_dims("c2n20a"))])
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    multi = [_take(w, r) for w, r in zip(ws, P.solve_fixed_multi(ws, lists))]
    print("NODEQPSOFT multi routes %s best %s" % ([list(m["route"]) for m in multi], [m["best"] for m in multi]))
    for h, (p, recs) in enumerate(zip(ps, lists)):
        twin = P.CplexWrapper(); twin.resetParameters(p)
        for k, r in enumerate(recs):
            _assert_entry_is_the_single_call("handle %d entry %d" % (h, k), multi[h], k, _single(twin, r))
        assert all(s == 0 for s in multi[h]["status"])
        assert multi[h]["best"] == min(range(len(recs)), key=lambda k: (multi[h]["objective"][k], k))
    # the same points ignored cost the same on either soft handle only where the rows were slack: the handles were told apart
    assert np.float64(multi[0]["objective"][0]).tobytes() != np.float64(multi[1]["objective"][0]).tobytes()


@pytest.mark.parametrize("name,mask,hard", [("c1n6r16hex", None, 0), ("c2n20a", (0, 1, 0, 0), 0), ("c2n20a", (0, 1, 0, 0), 2)], ids=["c1n6r16hex-hard", "c2n20a/0100-obstacle0", "c2n20a/0100-obstacle2"])
def test_an_ignored_mark_on_a_hard_obstacle_changes_nothing(oracle, name, mask, hard):
    """slack entry 1 at the odd steps of an obstacle whose obstacle_is_soft is 0, the deltacc zeros left as they were: device and oracle answer as
    for the unmarked record - the device with the unmarked case's bytes - and return the slack entries 0"""
    if mask is None:
        p, h, dims, rec = H.node_instance(oracle, name)
    else:
        p, h, dims, rec = H.soft_instance(oracle, name, mask)
    assert list(p.obstacle_is_soft)[hard] == 0
    marked = H.copy_record(rec)
    marked.slackvarsObstacle[:, hard, 1::2] = 1; marked.slackvarsObstacle_front[:, hard, 1::2, :] = 1
    assert marked.slackvarsObstacle.sum() > 0 and np.array_equal(marked.deltacc, rec.deltacc) and np.array_equal(marked.deltacc_front, rec.deltacc_front)
    o0, o1 = oracle.solve_fixed(h, dims, rec), oracle.solve_fixed(h, dims, marked)
    assert o0[0] == o1[0] == 0 and o0[2] == o1[2] and _soft_bytes(o0[1], o0[2]) == _soft_bytes(o1[1], o1[2])
    w = P.CplexWrapper(); w.resetParameters(p)
    d0, d1 = _single(w, rec), _single(w, marked)
    assert d0[0] == d1[0] == 0 and (d0[3], d0[4]) == (d1[3], d1[4])
    assert _soft_bytes(d0[1], d0[2]) == _soft_bytes(d1[1], d1[2])
    assert d1[1].slackvarsObstacle.sum() == 0 and d1[1].slackvarsObstacle_front.sum() == 0
    _assert_matches_oracle("%s marked on hard obstacle %d" % (name, hard), d1[0], d1[1], d1[2], o1[0], o1[1], o1[2])
    b = _take(w, w.solveFixedBatch([rec, marked]))
    assert _soft_bytes(b["records"][0], b["objective"][0]) == _soft_bytes(b["records"][1], b["objective"][1]) == _soft_bytes(d0[1], d0[2])

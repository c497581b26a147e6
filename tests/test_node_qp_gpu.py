"""The node QP kernels one node at a time: the device's solveFixed against the oracle's solve_fixed on partial fix records.

Every other device test runs a whole branch-and-bound solve; a node kernel that decodes one row class wrongly can still close on the same optimum
there.  Here each case is ONE continuous QP - the regions of a feasible record asserted, a chosen part of its leaf disjunctions undecided
(helpers.relax_levels) - solved by miqp_solver_solve_fixed (the serial interior point chain: standard on-chip block, larger on-chip block,
memory-backed kernel) and by the oracle's dense-row interior point to the same tolerance.  The number of decided disjunctions steers the
node through the chain, lastFixedRoute() says which launch solved it, and EXPECTED_ROUTE records where every case landed.

Of the eight row classes of the decode (cls_off / cls_cnt) seven are reached: state and input bounds, region rows, rear- and front-point edges of the
environment, obstacles, and the car/car rows of the fixed alternatives.  The eighth, the car/car EXCLUSION rows, cannot be reached through this entry:
they are switched on by the mask bytes at f_c2n of a fix record, which only the search writes for the later children of a branching; a RawResults
record has no field for them, fix_from_results leaves them at -1 (decode_row and slot_maybe then skip every slot of the class), and the oracle has no
row of that meaning.  They stay covered end to end only.

Soft obstacles - fix records that ignore points of an obstacle, the byte L and its price - are held against the oracle in the same way in
test_node_qp_soft_gpu.py.  The active-set kernels (solve_fixed runs the interior point chain only) are held against the oracle on the same records
in test_as_node_gpu.py.
All tests here need a real MI355X: run with  python -m pytest tests/test_node_qp_gpu.py -m gpu."""
import numpy as np
import pytest

import helpers as H
import planner_miqp_amd as P
from helpers import CONT_FIELDS

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-7     # the project's numbers for this pair of solvers at QP_TOL_FINAL (test_k3_fixed_binaries_on_device)
STATE_TOL = 1e-5
RAW_TOL = 1e-5      # violation of the raw big-M model, as the parity tests require

CASES = [(name, level) for name in H.NODE_SHAPES for level in H.level_names(H.shape_dims(name))]

# Which launch solved each case: 0 the standard on-chip block (up to OC_GCAP = 128 general rows), 1 the larger on-chip block (up to OC_GCAP_BIG = 320),
# 2 the memory-backed kernel behind them, 3 the memory-backed kernel of a shape without an on-chip kernel (more than 20 steps, three and four cars).
# Found on the device when the test was written; a shift of a capacity or of the number of rows the decode finds shows here.  With two cars the
# region rows alone fill the standard block from 8 steps on, so every level of "mini" and the region-only levels of cfg4's shape are the larger block's.
_NO_ONCHIP = ("c1n21o", "c1n40o", "mini3", "mini4", "c3n6o")
_CFG4 = ("c2n20a", "c2n20b", "c2n20c")
EXPECTED_ROUTE = {(name, level): 3 if name in _NO_ONCHIP else 0 for name, level in CASES}
EXPECTED_ROUTE.update({("mini", level): 1 for level in ("complete", "third", "two_thirds", "regions_only")})
EXPECTED_ROUTE.update({("c2n6e2pent", "complete"): 1, ("c2n6e2pent", "third"): 1})
EXPECTED_ROUTE.update({(name, level): 1 for name in _CFG4 for level in ("regions_only", "only_obs_rear", "only_c2c")})
EXPECTED_ROUTE.update({(name, level): 2 for name in _CFG4 for level in ("complete", "third", "two_thirds", "only_env_front", "only_obs_front")})

LEAF_FIELDS = H.ENV_FIELDS + ["deltacc", "deltacc_front", "car2car_collision"]
_WRAPPERS, _ORACLE, _ROUTES = {}, {}, {}


def _wrapper(oracle, name):
    if name not in _WRAPPERS:
        w = P.CplexWrapper(); w.resetParameters(H.node_instance(oracle, name)[0])
        _WRAPPERS[name] = w
    return _WRAPPERS[name]


def _case(oracle, name, level):
    """(record, oracle's rc, result, objective) of one case; computed once and left unchanged"""
    if (name, level) not in _ORACLE:
        p, h, dims, rec = H.node_instance(oracle, name)
        for lv, (r, decided) in H.relax_levels(rec, H.RELAX_SEED[name]).items():
            _ORACLE[(name, lv)] = (r,) + tuple(oracle.solve_fixed(h, dims, r)[:3])
    return _ORACLE[(name, level)]


def _device(oracle, name, record):
    w = _wrapper(oracle, name)
    rc, out, obj, it = w.solveFixed(record)
    return rc, out, obj, w.lastFixedRoute()


def _assert_matches_oracle(tag, rc, out, obj, ost, ores, oobj):
    assert rc == ost, (tag, rc, ost)
    if ost != 0:
        return
    diffs = {n: float(np.abs(getattr(out, n) - getattr(ores, n)).max()) for n in CONT_FIELDS}
    worst = max(diffs, key=diffs.get)
    print("NODEQP %s objective %.10f oracle %.10f rel %.2e worst state %s %.2e" % (tag, obj, oobj, abs(obj - oobj) / max(1.0, abs(oobj)), worst, diffs[worst]))
    assert abs(obj - oobj) <= OBJ_RTOL * max(1.0, abs(oobj)), (tag, obj, oobj)
    for n in CONT_FIELDS:
        assert diffs[n] <= STATE_TOL, (tag, n, diffs[n])


@pytest.mark.parametrize("name,level", CASES)
def test_node_matches_the_oracle(oracle, name, level):
    """same verdict; objective within 1e-7 relative and every continuous field within 1e-5 of the oracle's; the returned record asserts what the
    fix record asserted, and on the complete level it is feasible for the raw big-M model; the launch that solved the node is the recorded one"""
    record, ost, ores, oobj = _case(oracle, name, level)
    rc, out, obj, route = _device(oracle, name, record)
    _ROUTES[(name, level)] = route
    print("NODEQP %s/%s rc %d route %d" % (name, level, rc, route))
    assert ost == 0   # (test_node_records_cpu.py: every level is feasible for the oracle)
    _assert_matches_oracle("%s/%s" % (name, level), rc, out, obj, ost, ores, oobj)
    assert np.array_equal(out.active_region[:, 1:], record.active_region[:, 1:])
    for n in LEAF_FIELDS:   # (all of them [.., .., step, ..]; step 0 is constant and not part of a fix record)
        assert np.all(getattr(out, n)[:, :, 1:][getattr(record, n)[:, :, 1:] == 0] == 0), (name, level, n)
    if level == "complete":
        v, robj, worst = oracle.raw_eval(H.node_instance(oracle, name)[1], out)
        print("NODEQP %s/%s raw-model violation %.2e (%s)" % (name, level, v, worst))
        assert v < RAW_TOL and abs(robj - obj) <= 1e-6 * max(1.0, abs(obj)), (name, worst, robj, obj)
    assert route == EXPECTED_ROUTE[(name, level)], (name, level, route)


@pytest.mark.parametrize("k", range(len(H.INFEASIBLE_NODES)))
def test_infeasible_node_is_reported_and_leaves_nothing_behind(oracle, k):
    """a grossly infeasible node (step 1 on the wrong side of an obstacle or of the other car) gets verdict 1, and the next feasible node on the
    same handle is answered as if it had not been there"""
    name, cls, key, alt = H.INFEASIBLE_NODES[k]
    p, h, dims, rec = H.node_instance(oracle, name)
    bad = H.infeasible_record(rec, cls, key, alt)
    assert oracle.solve_fixed(h, dims, bad)[0] == 1
    rc, out, obj, route = _device(oracle, name, bad)
    print("NODEQP infeasible %s %s %s -> %d: rc %d route %d" % (name, cls, key, alt, rc, route))
    assert rc == 1, (name, cls, key, alt, rc)
    level = H.level_names(dims)[k % 4]   # (complete, third, two_thirds, regions_only in turn)
    record, ost, ores, oobj = _case(oracle, name, level)
    rc, out, obj, route = _device(oracle, name, record)
    _assert_matches_oracle("%s/%s after an infeasible node" % (name, level), rc, out, obj, ost, ores, oobj)
    assert route == EXPECTED_ROUTE[(name, level)]


def _bytes(out, obj):
    return b"".join(np.ascontiguousarray(getattr(out, n)).tobytes() for n in CONT_FIELDS + H.BIN_FIELDS + ["car2car_collision", "slackvars_real"]) + np.float64(obj).tobytes()


@pytest.mark.parametrize("route", [0, 1, 2, 3])
def test_one_node_of_each_route_is_bit_stable(oracle, route):
    name, level = next(c for c in CASES if EXPECTED_ROUTE[c] == route and c[1] != "complete")
    record = _case(oracle, name, level)[0]
    other = _case(oracle, name, "complete")[0]
    rc1, out1, obj1, r1 = _device(oracle, name, record)
    _device(oracle, name, other)   # (another node in between: nothing of it may stay)
    rc2, out2, obj2, r2 = _device(oracle, name, record)
    assert rc1 == rc2 == 0 and r1 == r2 == route
    assert _bytes(out1, obj1) == _bytes(out2, obj2)


def test_every_route_of_the_chain_is_reached(oracle):
    """each launch of the chain solves at least three cases, and cfg4's shape - the only one that crosses both on-chip capacities - reaches the
    larger block and the memory-backed kernel behind it: a capacity change that empties a route fails here"""
    for name, level in CASES:
        if (name, level) not in _ROUTES:   # (the cases were not run in this session: only their routes are needed)
            _ROUTES[(name, level)] = _device(oracle, name, _case(oracle, name, level)[0])[3]
    count = {r: sum(1 for v in _ROUTES.values() if v == r) for r in (0, 1, 2, 3)}
    print("NODEQP cases per route", count)
    assert all(count[r] >= 3 for r in (0, 1, 2, 3)), count
    for r in (1, 2):
        assert any(v == r and name.startswith("c2n20") for (name, level), v in _ROUTES.items()), (r, count)
    assert all(v in (0, 1, 2, 3) for v in _ROUTES.values()) and set(_ROUTES) == set(CASES)

"""The dual active-set node kernel one node at a time: CplexWrapper.solveFixedActiveSet against the oracle's solve_fixed on partial fix records.

Every other test that runs as_onchip_kernel runs a whole branch and bound and compares the incumbent, which the interior point has polished; a
search forgives this kernel a node it cannot finish, a parent's M that no longer fits, a wrong verdict on a subtree that did not hold the optimum.
Here each case is ONE continuous QP - the records of helpers.relax_levels, pinned for the oracle in test_node_records_cpu.py and
test_as_node_records_cpu.py - sent through ONE launch of the standard or of the larger block (miqp_solver_solve_fixed_as: kernel, LDS size and
grid are the round planner's), cold, from a parent's final active set with its M, or from that set with M rebuilt, with and without a cutoff, and
what the kernel decided is read back as it wrote it.  The reference is always oracle.solve_fixed on the same record (the cache of
test_node_qp_gpu.py), never another device run.

Not reached through this entry, as in test_node_qp_gpu.py: the car/car EXCLUSION rows (mask bytes only the search writes), the region SETS and the
hull boxes of undecided regions (a RawResults record decides every region).  The oracle has no rows of those meanings; they stay covered end to end.

MEASURED on an MI355X over all 547 solved nodes of this file (cold, started, soft; both blocks), against the oracle (profiles/as_node_pin.txt):
  worst relative objective deviation 3.25e-12 and worst state deviation 3.45e-9 (u_y), both on c2n20w107/only_c2c cold on the larger block (45 active
  rows, 93 steps); worst reported violation 3.0e-11.  The tolerances below are ten times those, far inside the caps of 1e-6 and 1e-4.
STATUS per block follows EXPECTED_ROUTE of test_node_qp_gpu.py without exception (route 0: solved by both blocks, 1: status 3 on the standard
  block and solved on the larger one, 2: status 3 on both); LARGE_ROUTE below is that table for the two shapes with large active sets.
FALL-BACKS to a cold start: none, in the first generation and in the later ones of the chain, on every shape and both blocks.
STEPS of the started children of all chains and pairs together 395, of the same records cold 846.
FULL SLOTS: c2n20f11 (98 active rows for the oracle on only_c2c, 66 on regions_only) comes back 4 from the larger block on both levels, reason "no free
  slot" and no other, cold and started; solveFixed matches the oracle's objective on it to 1.6e-12 relative.
NOT COVERED: the load of a parent's packed triangle in more than one part - the largest finished parent here has 48 rows, whose 1176 doubles fit the
  larger block's staging room of 1184 (helpers.py has the count per block and the search for a larger well-posed parent).
FINDING: the kernel tests the cutoff after a step.  A node it solves WITHOUT a step - no row violated at the unconstrained optimum: c1n2r16,
  c1n3r32, regions_only and only_obs_rear of c1n2r32o - is never tested and comes back solved, its objective above the cutoff; in a search
  eval_kernel drops such a node by its bound ("bound not better than the incumbent").  test_cutoff_* asserts exactly that for those nodes.
All tests here need a real MI355X: run with  python -m pytest tests/test_as_node_gpu.py -m gpu."""
import numpy as np
import pytest

import helpers as H
import planner_miqp_amd as P
from helpers import CONT_FIELDS
from test_node_qp_gpu import EXPECTED_ROUTE, LEAF_FIELDS, _case

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-7       # the project's number for two solvers of one QP (test_node_qp_gpu.py); here the bound of weak duality: bound <= oracle * (1 + OBJ_RTOL)
VIOL_TOL = 5e-7       # the kernel's own acceptance of an iterate
RAW_TOL = 1e-5        # violation of the raw big-M model, as the parity tests require
AS_OBJ_RTOL = 3.3e-11   # objective of the unpolished iterate against the oracle: ten times the worst measured (cap: 1e-6, the project's number for
AS_STATE_TOL = 3.5e-8   # active set against interior point in test_one_car_active_set_gpu.py); states likewise (cap: 1e-4)
assert AS_OBJ_RTOL <= 1e-6 and AS_STATE_TOL <= 1e-4
SLOTS = 64            # rows the method holds

SHAPES = H.as_shapes()
CASES = [(name, level) for name in SHAPES for level in H.level_names(H.shape_dims(name))]
_DATA, _WRAPPERS = {}, {}


def _wrapper(oracle, name):
    if name not in _WRAPPERS:
        w = P.CplexWrapper(); w.resetParameters(H.node_instance(oracle, name)[0])
        _WRAPPERS[name] = w
    return _WRAPPERS[name]


# where the interior point chain solves the levels of the shapes with large active sets (found on the device, as EXPECTED_ROUTE was)
# (cfg3's shape: the front-point rows of its two environment pieces are beyond both blocks, as on cfg4's; the regions alone and with the car/car rows are the larger block's)
LARGE_ROUTE = {(name, level): 1 if level in ("regions_only", "only_c2c") else 2 for name in H.AS_LARGE_SHAPES for level in H.level_names(H.shape_dims(name))}
ROUTE = {**EXPECTED_ROUTE, **LARGE_ROUTE}


# The one start pair whose parent ends with an active row that the child does not have: front points 1 and 3 of c1n2r32o's obstacle give the same
# binding row, the complete record's solve keeps it under the identity it meets first, and two_thirds decides point 3 alone
# (test_as_node_records_cpu.py::test_the_one_start_pair_whose_child_keeps_no_row_of_its_parent shows it from the oracle)
NO_SHARED_ROW = {("c1n2r32o", "complete", "two_thirds")}


def _held(D, level, block):
    """whether the block holds the node's rows: where the interior point chain solved the same record (both kernels include the one decode)"""
    return D["route"][level] <= block


def _node_bytes(w, nodes, k):
    rc, rec = w.fixedActiveSetRecord(k)
    b = nodes[k:k + 1].tobytes()
    if rc == 0:
        b += b"".join(np.ascontiguousarray(getattr(rec, n)).tobytes() for n in CONT_FIELDS + H.BIN_FIELDS + ["car2car_collision", "slackvars_real"])
    return b


class Call:
    """one call of the entry: its nodes, its counters, and the bytes and records of the nodes asked for"""

    def __init__(self, w, records, start=None, block=0, cutoff=None, keep=()):
        try:
            self.nodes, self.info = w.solveFixedActiveSet(records, start=start, block=block, cutoff=cutoff)
        except RuntimeError as e:
            if "(-3)" in str(e):   # a HIP error: nothing more is started on the device in this session
                pytest.exit("solveFixedActiveSet: %s" % e, returncode=3)
            raise
        self.bytes = {k: _node_bytes(w, self.nodes, k) for k in keep}
        self.rec = {k: w.fixedActiveSetRecord(k)[1] for k in keep}


def _starts(levels, name, rebuilt):
    """records and start words of the first-generation pairs and of the chain: the levels cold in front (node q is level q), then the children"""
    names = list(levels)
    recs = [levels[n][0] for n in names]
    start = [-1] * len(names)
    pairs = []   # (parent node, child node, parent level, child level, generation)
    word = (lambda p: -(p + 2)) if rebuilt else (lambda p: p)
    for a, b in H.as_first_pairs(name):
        recs.append(levels[b][0]); start.append(word(names.index(a))); pairs.append((names.index(a), len(recs) - 1, a, b, 1))
    first = len(recs)
    if len(names) > 1:
        prev = names.index(H.AS_CHAIN[0])
        for g, b in enumerate(H.AS_CHAIN[1:]):
            recs.append(levels[b][0]); start.append(word(prev)); pairs.append((prev, len(recs) - 1, H.AS_CHAIN[g], b, g + 1)); prev = len(recs) - 1
    return recs, start, pairs, first


def _data(oracle, name):
    """everything the device is asked about a shape, once per session: the calls of a shape follow each other, so the device context is built once"""
    if name in _DATA:
        return _DATA[name]
    p, h, dims, rec = H.node_instance(oracle, name)
    levels = H.relax_levels(rec, H.RELAX_SEED[name])
    names = list(levels)
    recs = [levels[n][0] for n in names]
    w = _wrapper(oracle, name)
    D = {"names": names, "dims": dims, "route": {}, "cold": {}, "cut": {}, "first": {}, "chain": {}, "again": {}, "verdict": {}}
    for n in names:   # (the interior point chain on the same records: where each was solved)
        w.solveFixed(levels[n][0]); D["route"][n] = w.lastFixedRoute()
    orc = {n: _case(oracle, name, n) for n in names}
    for block in (0, 1):
        keep = range(len(names))
        D["cold"][block] = cold = Call(w, recs, block=block, keep=keep)
        solved = [q for q in range(len(names)) if cold.nodes["status"][q] == 0]
        # cutoffs: 1e-3 below and above the oracle's objective - four orders above every tolerance involved, so neither side is a tie
        cr = [recs[q] for q in solved] * 2
        cc = [orc[names[q]][3] * (1 - 1e-3) for q in solved] + [orc[names[q]][3] * (1 + 1e-3) for q in solved]
        D["cut"][block] = (solved, Call(w, cr, block=block, cutoff=cc, keep=range(len(solved), 2 * len(solved))) if solved else None)
        for rebuilt in (False, True):
            r2, st, pairs, first = _starts(levels, name, rebuilt)
            if not pairs:
                continue
            # (the first generation alone, then the whole list: the counters of a call are sums over its launches)
            D["first"][(block, rebuilt)] = (pairs[:first - len(names)], Call(w, r2[:first], start=st[:first], block=block, keep=range(len(names), first)))
            D["chain"][(block, rebuilt)] = (pairs, Call(w, r2, start=st, block=block, keep=range(len(names), len(r2))))
        if (block, False) in D["first"]:   # a warm child in two separate calls
            r2, st, pairs, first = _starts(levels, name, False)
            D["again"][block] = Call(w, r2[:first], start=st[:first], block=block, keep=range(len(names), first))
        D["verdict"][block] = []
        for lv0 in sorted({lv for n, lv, cls, key, alt in H.AS_INFEASIBLE if n == name}):   # (each record with the level it was made from)
            bad = [H.infeasible_record(levels[lv0][0], cls, key, alt) for n, lv, cls, key, alt in H.AS_INFEASIBLE if n == name and lv == lv0]
            vr = [levels[lv0][0]] + bad + bad + [levels[lv0][0]]
            vs = [-1] + [-1] * len(bad) + [0] * len(bad) + [-1]
            D["verdict"][block].append((lv0, len(bad), Call(w, vr, start=vs, block=block, keep=(0, len(vr) - 1))))
    _DATA[name] = D
    return D


def _against_oracle(tag, node, rec, orc, record, oracle=None, raw_handle=None):
    """a solved node against the oracle's answer on the same record: the conditions of a cold solve.  Returns (relative objective deviation, worst state deviation)"""
    ost, ores, oobj = orc[1], orc[2], orc[3]
    assert ost == 0
    assert node["status"] == 0, (tag, int(node["status"]))
    rel = abs(node["objective"] - oobj) / max(1.0, abs(oobj))
    diffs = {n: float(np.abs(getattr(rec, n) - getattr(ores, n)).max()) for n in CONT_FIELDS}
    worst = max(diffs, key=diffs.get)
    print("ASNODE %s objective %.10f bound %.10f oracle %.10f rel %.2e viol %.1e steps %d active %d worst state %s %.2e"
          % (tag, node["objective"], node["bound"], oobj, rel, node["violation"], node["steps"], node["active"], worst, diffs[worst]))
    assert node["bound"] <= oobj * (1 + OBJ_RTOL), (tag, float(node["bound"]), oobj)   # weak duality
    assert node["bound"] <= node["objective"]
    assert 0 <= node["violation"] <= VIOL_TOL, (tag, float(node["violation"]))
    assert 0 <= node["active"] <= SLOTS
    assert rel <= AS_OBJ_RTOL, (tag, float(node["objective"]), oobj, rel)
    assert diffs[worst] <= AS_STATE_TOL, (tag, worst, diffs[worst])
    assert np.array_equal(rec.active_region[:, 1:], record.active_region[:, 1:])
    for n in LEAF_FIELDS:
        assert np.all(getattr(rec, n)[:, :, 1:][getattr(record, n)[:, :, 1:] == 0] == 0), (tag, n)
    if raw_handle is not None:
        v, robj, wr = oracle.raw_eval(raw_handle, rec)
        assert v < RAW_TOL and abs(robj - node["objective"]) <= 1e-6 * max(1.0, abs(node["objective"])), (tag, wr, v, robj)
    return rel, diffs[worst]


@pytest.mark.parametrize("name,level", CASES)
def test_cold_node_matches_the_oracle_on_the_block_that_holds_it(oracle, name, level):
    """status 3 exactly where the interior point chain handed the record on (route 0: both blocks solve it, 1: the larger one, 2: neither); on the
    blocks that hold it the node is solved - never 4 with the 48 active rows or fewer of these cases, never 1 - its bound lies below the oracle's
    objective, its violation within the kernel's acceptance, objective and states within the measured tolerances, the returned record asserts what the
    fix record asserted and, on the complete level, is feasible for the raw model"""
    D = _data(oracle, name)
    q = D["names"].index(level)
    orc = _case(oracle, name, level)
    route = D["route"][level]
    assert route == ROUTE[(name, level)], (name, level, route)
    for block in (0, 1):
        c = D["cold"][block]
        node = c.nodes[q]
        print("ASNODE %s/%s block %d route %d status %d" % (name, level, block, route, node["status"]))
        if route > block:
            assert node["status"] == 3, (name, level, block, int(node["status"]))
            continue
        _against_oracle("%s/%s block %d cold" % (name, level, block), node, c.rec[q], orc, orc[0], oracle, H.node_instance(oracle, name)[1] if level == "complete" else None)
    if route == 0:   # the two blocks run one method on one set of rows
        a, b = D["cold"][0].nodes[q], D["cold"][1].nodes[q]
        assert abs(a["objective"] - b["objective"]) <= 2 * AS_OBJ_RTOL * max(1.0, abs(a["objective"]))


@pytest.mark.parametrize("name", SHAPES)
def test_cutoff_below_cuts_the_node_off_and_above_changes_nothing(oracle, name):
    """every solved cold case again with a cutoff 1e-3 below the oracle's objective - status 2 with cutoff < bound <= oracle * (1 + 1e-7) - and 1e-3
    above it: status 0 and the bytes of the solve without a cutoff.  A node solved without a step has no test of the cutoff (FINDING in the header):
    it comes back solved under either cutoff, with the same bytes"""
    D = _data(oracle, name)
    for block in (0, 1):
        solved, c = D["cut"][block]
        for j, q in enumerate(solved):
            level = D["names"][q]
            oobj = _case(oracle, name, level)[3]
            lo, hi = c.nodes[j], c.nodes[len(solved) + j]
            print("ASNODE %s/%s block %d cutoff below: status %d bound %.10f steps %d; above: status %d" % (name, level, block, lo["status"], lo["bound"], lo["steps"], hi["status"]))
            assert hi["status"] == 0 and c.bytes[len(solved) + j] == D["cold"][block].bytes[q], (name, level, block)
            if D["cold"][block].nodes[q]["steps"] == 0:
                # solved without a step: the kernel's test comes after a step, so this node is never tested (the evaluation drops it by its bound)
                assert lo["status"] == 0 and lo["steps"] == 0 and lo["objective"] > oobj * (1 - 1e-3) and c.nodes[j:j + 1].tobytes() == hi.tobytes(), (name, level, block)
                continue
            assert lo["status"] == 2, (name, level, block, int(lo["status"]))
            assert oobj * (1 - 1e-3) < lo["bound"] <= oobj * (1 + OBJ_RTOL), (name, level, block, float(lo["bound"]), oobj)


def _children(oracle, name, D, kind, block, rebuilt):
    pairs, c = D[kind][(block, rebuilt)]
    cold = D["cold"][block]
    out = []
    for pn, cn, a, b, g in pairs:
        if not _held(D, b, block):
            assert c.nodes[cn]["status"] == 3
            continue
        orc = _case(oracle, name, b)
        tag = "%s %s->%s block %d %s generation %d" % (name, a, b, block, "M rebuilt" if rebuilt else "parent's M", g)
        _against_oracle(tag, c.nodes[cn], c.rec[cn], orc, orc[0])
        cq = cold.nodes[D["names"].index(b)]
        assert abs(c.nodes[cn]["objective"] - cq["objective"]) <= 2 * AS_OBJ_RTOL * max(1.0, abs(cq["objective"])), tag
        out.append((pn, cn, a, b, g))
    return out, c


@pytest.mark.parametrize("name", [n for n in SHAPES if H.as_first_pairs(n)])
def test_started_nodes_match_the_oracle_and_the_counters_say_how_they_started(oracle, name):
    """rows arrive (regions_only -> two_thirds), rows leave (complete -> two_thirds: down-dates), each class on its own (regions_only -> only_*), and
    the chain regions_only -> two_thirds -> third -> complete over three generations; each once with the parent's M and once with the tag cleared.
    Every child the block holds is checked against the oracle exactly as a cold solve is, and against its own cold result.  Counters of the first
    generation: with M the nodes started from the parent's M EQUAL the children whose parent ended with an active row, none fell back to a cold
    start, rows were taken over wherever a child started; with the tag cleared the reason "the parent left none" counts those children.  One
    exception, named in NO_SHARED_ROW and explained from the reference in test_as_node_records_cpu.py: c1n2r32o's complete -> two_thirds, whose
    child has none of its parent's rows.  Later generations: the fall-backs are printed, not asserted (measured: none)."""
    D = _data(oracle, name)
    for block in (0, 1):
        for rebuilt in (False, True):
            held, c = _children(oracle, name, D, "first", block, rebuilt)
            info = [int(v) for v in c.info]
            # children whose parent ended with an active row: each starts from it - but for the ONE pair whose child keeps no row of its parent
            # (NO_SHARED_ROW): `if (u0)` in the kernel then skips the start and every counter of it
            warm = [x for x in held if c.nodes[x[0]]["status"] == 0 and c.nodes[x[0]]["active"] >= 1]
            expect = [x for x in warm if (name, x[2], x[3]) not in NO_SHARED_ROW]
            print("ASNODE %s block %d %s first generation: children held %d, with a parent set %d (expected to start from it: %d), from M %d, fell back %d, rows taken over %d, rebuilt (no ring %d, parent left none %d, ring round %d, other count %d)"
                  % (name, block, "M rebuilt" if rebuilt else "parent's M", len(held), len(warm), len(expect), info[8], info[9], info[7], info[16], info[17], info[18], info[19]))
            assert info[9] == 0, (name, block, rebuilt, info[9])
            started = info[17] if rebuilt else info[8]
            assert started == len(expect), (name, block, rebuilt, started, len(expect), len(warm))
            assert (info[8] == 0 and info[16] == info[18] == info[19] == 0) if rebuilt else info[16:20] == [0, 0, 0, 0], (name, block, rebuilt, info[8], info[16:20])
            assert (info[7] > 0) == (len(expect) > 0), (name, block, rebuilt, info[7], len(expect))
            held2, c2 = _children(oracle, name, D, "chain", block, rebuilt)
            i2 = [int(v) for v in c2.info]
            print("ASNODE %s block %d %s chain and pairs: children held %d, from M %d, fell back %d (later generations: %d)" % (name, block, "M rebuilt" if rebuilt else "parent's M", len(held2), i2[8], i2[9], i2[9] - info[9]))


def test_warm_starts_save_steps_over_all_pairs(oracle):
    """over all pairs and chains of all shapes together, the children started from their parent's M take fewer steps than the same records cold"""
    warm = cold = 0
    for name in SHAPES:
        if not H.as_first_pairs(name):
            continue
        D = _data(oracle, name)
        for block in (0, 1):
            pairs, c = D["chain"][(block, False)]
            for pn, cn, a, b, g in pairs:
                if c.nodes[cn]["status"] == 0:
                    warm += int(c.nodes[cn]["steps"]); cold += int(D["cold"][block].nodes[D["names"].index(b)]["steps"])
    print("ASNODE steps of the started children %d, of the same records cold %d" % (warm, cold))
    assert 0 < warm < cold


@pytest.mark.parametrize("name", sorted({n for n, lv, cls, key, alt in H.AS_INFEASIBLE}))
def test_infeasible_records_are_called_infeasible_and_leave_nothing_behind(oracle, name):
    """step 1 on the wrong side of an obstacle or of the other car: status 1 cold and started from the feasible record it was made from, on every
    block that holds the record; the feasible record behind them in the same call is answered with the bytes it had in front of them"""
    D = _data(oracle, name)
    some = False
    for block in (0, 1):
        for lv0, nbad, c in D["verdict"][block]:
            st = [int(v) for v in c.nodes["status"]]
            print("ASNODE %s block %d verdicts on %s: %s" % (name, block, lv0, st))
            if not _held(D, lv0, block):
                assert st == [3] * len(st)
                continue
            some = True
            assert st[0] == 0 and st[-1] == 0 and st[1:-1] == [1] * (2 * nbad), (name, block, st)
            assert c.bytes[0] == c.bytes[len(st) - 1] == D["cold"][block].bytes[D["names"].index(lv0)]
    assert some


def test_no_feasible_case_is_called_infeasible_or_left_unfinished(oracle):
    """over every call of this file: a feasible record never comes back 1, and with the 48 rows or fewer of these cases never 4"""
    for name in SHAPES:
        D = _data(oracle, name)
        for block in (0, 1):
            calls = [D["cold"][block]] + [D[k][key][1] for k in ("first", "chain") for key in D[k] if key[0] == block] + ([D["again"][block]] if block in D["again"] else [])
            for c in calls:
                assert set(int(v) for v in c.nodes["status"]) <= {0, 3}, (name, block, c.nodes["status"])
            info = [int(v) for v in D["cold"][block].info]
            assert info[2] == 0 and info[4] == 0 and info[10:16] == [0] * 6, (name, block, info)


@pytest.mark.parametrize("name,block,level", [("c1n6r32o", 0, "third"), ("mini", 1, "third")])
def test_a_node_is_bit_stable_whatever_its_place_and_neighbours(oracle, name, block, level):
    """identical bytes of every output alone, as slots 0 and 700 of a call among other records, as 65 copies in one call; a warm child in two separate calls"""
    D = _data(oracle, name)
    w = _wrapper(oracle, name)
    levels = H.relax_levels(H.node_instance(oracle, name)[3], H.RELAX_SEED[name])
    r = levels[level][0]
    ref = D["cold"][block].bytes[D["names"].index(level)]
    assert D["cold"][block].nodes[D["names"].index(level)]["status"] == 0
    alone = Call(w, [r], block=block, keep=(0,))
    others = [levels[n][0] for n in D["names"]]
    among = Call(w, [r] + [others[k % len(others)] for k in range(699)] + [r], block=block, keep=(0, 700))
    copies = Call(w, [r] * 65, block=block, keep=range(65))
    assert alone.bytes[0] == ref and among.bytes[0] == ref and among.bytes[700] == ref
    assert all(copies.bytes[k] == ref for k in range(65))
    pairs, c = D["first"][(block, False)]
    again = D["again"][block]
    assert pairs and all(c.bytes[cn] == again.bytes[cn] for pn, cn, a, b, g in pairs)


@pytest.mark.parametrize("name", list(H.AS_FULL_SHAPES))
def test_full_slots_come_back_unfinished_with_their_reason(oracle, name):
    """a node that needs more active rows than the 64 slots (the oracle: 98 on only_c2c, 66 on regions_only) comes back 4 from the block that holds
    it, with the reason "no free slot" and no other - never solved, never infeasible - cold and started from the other level; the standard block
    returns it as too large (3); and the interior point's solveFixed still matches the oracle's objective on it.  Only the level with 72 rows or
    more is asserted to be 4: 66 is too close to 64 for the oracle's count to decide (its status is printed, and is never 1).  The shape is exempt
    from the state rule (helpers.py, FULL SLOTS): no state is compared."""
    p, h, dims, rec = H.node_instance(oracle, name)
    levels = H.relax_levels(rec, H.RELAX_SEED[name])
    w = _wrapper(oracle, name)
    big, edge = levels["only_c2c"][0], levels["regions_only"][0]
    for lv, r in (("only_c2c", big), ("regions_only", edge)):
        ost, ores, oobj, oit = oracle.solve_fixed(h, dims, r)
        rc, out, obj, it = w.solveFixed(r)
        print("ASNODE %s/%s solveFixed rc %d route %d objective %.8f oracle %.8f rel %.1e" % (name, lv, rc, w.lastFixedRoute(), obj, oobj, abs(obj - oobj) / oobj))
        assert ost == 0 and rc == 0 and w.lastFixedRoute() == 1 and abs(obj - oobj) <= OBJ_RTOL * abs(oobj), (name, lv, rc, obj, oobj)
    assert Call(w, [big, edge], block=0).nodes["status"].tolist() == [3, 3]
    c = Call(w, [big], block=1)
    info = [int(v) for v in c.info]
    print("ASNODE %s/only_c2c block 1 cold status %d counters: finished %d unfinished %d reasons %s" % (name, c.nodes[0]["status"], info[0], info[2], info[10:16]))
    assert c.nodes[0]["status"] == 4 and np.isnan(c.nodes[0]["objective"]) and c.nodes[0]["active"] == 0
    assert info[0] == 0 and info[2] == 1 and info[10:16] == [0, 1, 0, 0, 0, 0], info[:20]   # ([11]: no free slot)
    c2 = Call(w, [edge, big, big], start=[-1, 0, -2], block=1)   # (from the other level's final set, with its M and with M rebuilt - if that level was finished)
    i2 = [int(v) for v in c2.info]
    print("ASNODE %s regions_only cold status %d steps %d active %d; only_c2c started from it: %s; reasons %s" % (name, c2.nodes[0]["status"], c2.nodes[0]["steps"], c2.nodes[0]["active"], c2.nodes["status"][1:].tolist(), i2[10:16]))
    assert c2.nodes[0]["status"] in (0, 4) and c2.nodes["status"][1:].tolist() == [4, 4]
    assert i2[11] == i2[2] >= 2 and i2[10] == 0 and i2[12:16] == [0, 0, 0, 0], i2[:20]


_SOFT = [(n, m) for n, m in H.SOFT_CASES if n in SHAPES]


@pytest.mark.parametrize("name,mask", _SOFT, ids=[H.soft_tag(n, m) for n, m in _SOFT])
def test_soft_levels_match_the_oracle_with_the_price_of_the_ignored_points(oracle, name, mask):
    """fix records that ignore points of a soft obstacle (byte L): the objective, with the price of the ignored points, and the states against the
    oracle's on the same record, on every block that holds the node.  (The car/car rows - quadratic-soft rows, whose 1/a term enters the
    method's S_pp and its residual - bind on 'complete' of mini and 'only_c2c' of c2n6e2pent among the cold cases above.)
    On cfg4's shape (c2n20a/0100, c2n20a/1000, c2n20b/0100) every soft level is made from the complete record and is beyond both blocks: for those
    three cases this test says nothing about the method - it asserts that both blocks return the node unsolved (status 3) where the interior
    point chain handed it on."""
    p, h, dims, rec = H.soft_instance(oracle, name, mask)
    w = P.CplexWrapper(); w.resetParameters(p)
    levels = H.soft_levels(name, rec, mask)
    recs = [levels[lv][0] for lv in H.SOFT_LEVELS]
    orc = [(r,) + tuple(oracle.solve_fixed(h, dims, r)[:3]) for r in recs]
    route = []
    for r in recs:   # (the interior point chain on the same records: which block holds each)
        w.solveFixed(r); route.append(w.lastFixedRoute())
    for block in (0, 1):
        c = Call(w, recs, block=block, keep=range(len(recs)))
        for q, lv in enumerate(H.SOFT_LEVELS):
            print("ASNODE %s %s block %d route %d status %d" % (H.soft_tag(name, mask), lv, block, route[q], c.nodes[q]["status"]))
            if route[q] > block:
                assert c.nodes[q]["status"] == 3
                continue
            _against_oracle("%s %s block %d" % (H.soft_tag(name, mask), lv, block), c.nodes[q], c.rec[q], orc[q], recs[q])
            assert H.ignored_points(c.rec[q]) == levels[lv][1]

"""The pools of many (source, destination) pairs carried in one device call (carry_solution_pools) against the single call.

Twin sets of fresh destinations built with the helpers of test_pool_carry_gpu.py: set A goes through carrySolutionPool pair by pair, set B through
ONE carry_solution_pools.  Per pair both sides agree bit for bit in the count, the dicts, the pool afterwards, last_timing out[2 .. 5] and
lastError().  The single call is itself pinned against its host replay in test_pool_carry_gpu.py, so the reference here is that call and nothing
else.  The sources are the shared ones of that file (solved under filter 12 and explored, settled); a destination is synthetic.advance of its
source along the source's solution, solved on a fresh wrapper - or only loaded (an EMPTY destination), or solved at capacity 1 (a FULL one).
Every solve of a comparison runs in front of its pool calls: a solve and a pool call size the device context differently.
The shapes are the smallest at which each per-pair quantity - maps, p_src, n0, ns, K, obj0, the first record - differs between neighbours in one
call.  By DESIGN.md 6l the single call admits on cfg4 seeds 12 and 5 and on an empty destination of c2n6e2pent; a comparison in which set A admits
on fewer pairs than it says FAILS, it does not skip.
All tests here need a real MI355X: run with  python -m pytest tests/test_pool_carry_multi_gpu.py -m gpu -s."""
import ctypes as C

import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd.ctypes_types import PoolCarryC
from test_pool_carry_gpu import _dst, _dst_params, _fresh_dst, _pool, _source
from test_pool_explore_gpu import _same_solve, _timing
from test_pool_filter_gpu import FILTER, _as_found

pytestmark = pytest.mark.gpu

# a pair: (source case, its capacity, the destination's variant, the destination's capacity or None for the source's, solved)
S12, S12X, S10, S5, S5FULL, S12EMPTY = (("cfg4s12", 16, "plain", None, True), ("cfg4s12", 16, "extra", None, True), ("cfg4s10", 16, "plain", None, True),
                                        ("cfg4s5", 16, "plain", None, True), ("cfg4s5", 16, "plain", 1, True), ("cfg4s12", 16, "plain", None, False))
CFG4 = [S12, S12X, S10, S5FULL, S5, S12EMPTY]   # (the full destination in the middle)
PENT = [("c2n6e2pent", 8, "plain", None, True), ("c2n6e2pent", 8, "without", None, True), ("c2n6e2pent", 8, "plain", None, False)]
WRAP = [("wrap", 8, "plain", None, True), ("wrap", 8, "extra", None, True), ("wrap", 8, "plain", None, False)]
_A, _B = {}, {}


def _fresh(item, shift):
    name, cap, variant, dcap, solve = item
    return _fresh_dst(name, cap, shift, variant, dcap, solve)


def _pbytes(w):
    p = _pool(w)
    return (p["n"], np.asarray(p["found"], dtype=np.float64).tobytes(), [x.tobytes() for x in p["dec"]])


def _snap(d, rc, out, before):
    """what a pair shows behind its call; the destination's old entries are the same bytes in the same places"""
    w = d["w"]
    p = _pool(w)
    t = _timing(w)
    assert p["n"] == d["n"] + max(rc, 0) and [x.tobytes() for x in p["dec"][:d["n"]]] == [x.tobytes() for x in d["dec"]]
    assert np.asarray(p["found"][:d["n"]], dtype=np.float64).tobytes() == np.asarray(d["found"], dtype=np.float64).tobytes()
    return dict(rc=rc, out=[sorted((k, np.float64(v).tobytes() if k == "objective" else v) for k, v in o.items()) for o in out], statuses=[o["status"] for o in out], n0=d["n"],
                pool=(p["n"], np.asarray(p["found"], dtype=np.float64).tobytes(), [x.tobytes() for x in p["dec"]]), timing=t[2:6], idle=t == before, err=w.lastError())


def _same_pair(a, b, what):
    """what the issue compares per pair; a pair that took no part keeps the whole last timing it had on either side"""
    for k in ("rc", "out", "n0", "pool", "err", "idle"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    if not a["idle"]:
        assert a["timing"] == b["timing"], (what, a["timing"], b["timing"])


def _compare(spec, shift=1, max_rel=-1.0, adding=2, keep=True):
    """set A (shared between the comparisons: a single call does not depend on the set it stands in) and a fresh set B through one call"""
    for name, cap in dict.fromkeys((s[0], s[1]) for s in spec):
        _source(name, cap)
    todo = [s for s in dict.fromkeys(spec) if (s, shift, max_rel) not in _A]
    da, db = [_fresh(s, shift) for s in todo], [_fresh(s, shift) for s in spec]
    for s, d in zip(todo, da):
        t0 = _timing(d["w"])
        rc, out = d["w"].carrySolutionPool(_source(s[0], s[1])["w"], shift, max_rel)
        _A[(s, shift, max_rel)] = _snap(d, rc, out, t0)
    t0 = [_timing(d["w"]) for d in db]
    res = P.carry_solution_pools([d["w"] for d in db], [_source(s[0], s[1])["w"] for s in spec], shift, max_rel)
    last = P.pool_carry_multi_last()
    b = [_snap(d, rc, out, t) for d, (rc, out), t in zip(db, res, t0)]
    a = [_A[(s, shift, max_rel)] for s in spec]
    print("CARRY MULTI shift %d max_rel %g: %d pairs, rounds %d, launch groups %d, device %.2f ms; admitted A %s B %s, statuses %s"
          % (shift, max_rel, len(spec), last[0], last[1], 1e3 * _timing(db[0]["w"])[1], [x["rc"] for x in a], [x["rc"] for x in b], [x["statuses"] for x in b]))
    for s, x, y in zip(spec, a, b):
        _same_pair(x, y, (s, shift, max_rel))
    assert sum(1 for x in a if x["rc"] > 0) >= adding, [x["rc"] for x in a]
    # the rounds of the call are those of its slowest pair, and all pairs of these sets fit one launch group a round
    assert last[0] == max(x["timing"][0] for x in b if not x["idle"]) == last[1]
    if keep:
        _B[(tuple(spec), shift, max_rel)] = b
    return a, b, db


@pytest.mark.parametrize("shift,max_rel", [(1, -1.0), (1, 0.5), (2, -1.0)], ids=["plain", "cap0.5", "shift2"])
def test_cfg4_pairs_in_one_call(shift, max_rel):
    a, b, _ = _compare(CFG4, shift, max_rel)
    assert a[3]["rc"] == 0 and a[3]["idle"] and a[3]["n0"] == 1   # (the full destination takes no part)
    assert a[5]["n0"] == 0 and (a[5]["rc"] >= 1 or shift != 1)   # (6l: the empty one admits at shift 1, whatever the cap)
    if shift == 1 and max_rel < 0:   # what 6l records for the single calls of seeds 12 and 5
        assert a[0]["rc"] >= 1 and a[4]["rc"] >= 1, [x["rc"] for x in a]
    assert len({tuple(x["timing"]) for x in b if not x["idle"]}) > 1   # (the pairs' own sums differ: they are not the call's)


def test_cfg4_pairs_in_reverse_order():
    first = _B.get((tuple(CFG4), 1, -1.0)) or _compare(CFG4)[1]
    a, b, _ = _compare(CFG4[::-1])
    for s, x, y in zip(CFG4, first, b[::-1]):   # every pair also gets the bits it got in the first order
        _same_pair(x, y, (s, "reverse"))


def test_one_source_feeds_two_destinations():
    s = _source("cfg4s12", 16)
    before = _pool(s["w"])
    a, b, _ = _compare([S12, S12EMPTY], adding=2)
    now = _pool(s["w"])
    assert now["n"] == before["n"] == s["n"] and np.asarray(now["found"]).tobytes() == np.asarray(s["found"]).tobytes()
    assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(now["dec"], before["dec"], s["dec"]))


def test_the_smallest_shape_with_unmappable_records():
    assert _dst_params("c2n6e2pent", 8, 1, "without") is not None
    a, b, _ = _compare(PENT, adding=1)
    assert a[1]["statuses"].count(2) == 7 and len(a[1]["statuses"]) == 8   # (6l: seven of eight records are unmappable)
    assert a[2]["rc"] >= 1 and a[2]["n0"] == 0                             # (6l: an empty destination admits its best feasible record)


def test_more_sites_than_lanes():
    """76 sites: the shift kernel's loop over the sites wraps past 64 lanes.  6l records no admission for wrap: statuses, solves, iterations and
    pools are compared, none is demanded"""
    a, b, db = _compare(WRAP, adding=0)
    rm, _ = db[1]["w"].poolCarryMaps(_source("wrap", 8)["w"])
    assert not np.array_equal(rm[0], np.arange(rm.shape[1]))
    assert all(len(x["statuses"]) == _source("wrap", 8)["n"] >= 1 for x in a)


def test_behind_the_call():
    spec = CFG4
    solved = [h for h, s in enumerate(spec) if s[4]]
    outside = _fresh(S12, 1)
    out0 = _pbytes(outside["w"]), _timing(outside["w"]), outside["w"].lastError()
    twins = [_fresh(s, 1) for s in spec]
    a, b, db = _compare(spec, keep=False)
    assert (_pbytes(outside["w"]), _timing(outside["w"]), outside["w"].lastError()) == out0   # a wrapper outside the call is untouched
    # two fresh B sets agree byte for byte
    first = _B.get((tuple(spec), 1, -1.0)) or _compare(spec)[1]
    for s, x, y in zip(spec, first, b):
        _same_pair(x, y, (s, "twin"))
    # the refinement leaves exactly L0 + added per destination, and every refined record certifies
    P.solve_solution_pools([twins[h]["w"] for h in solved])
    l0 = {h: twins[h]["w"].solutionPoolCount() for h in solved}
    ws = [db[h]["w"] for h in solved]
    res = P.solve_solution_pools(ws)
    for h, w, (st, obj, viol, it, route) in zip(solved, ws, res):
        assert len(obj) == w.solutionPoolCount() == l0[h] + a[h]["rc"], (spec[h], len(obj), l0[h], a[h]["rc"])
        for k in range(len(obj)):
            rc, rec = w.solutionPoolRecord(k)
            assert (rc == 0) == (st[k] == 0), (spec[h], k, rc, st[k])
            if rc == 0:
                cert = w.certify(rec)
                assert cert.status == 0 and cert.max_violation < 1e-5, (spec[h], k, cert)
        assert (st[l0[h]:] == 0).all()   # (a carried entry has settled labels: its own QP is feasible)
    assert all(r[0] >= 0 for r in P.improve_solution_pools(ws))   # the climb runs behind the call
    # a solve behind the call equals a fresh one
    for h in solved:
        s, w = spec[h], db[h]["w"]
        _same_solve(_dst(s[0], s[1], 1, s[2], s[3], s[4]), _as_found(w, w.callCplex()), (s, "a solve behind the call"))


def test_refusals_that_need_a_pool_leave_every_pool_alone():
    L = P.load_library()
    srcs = [_source("cfg4s12", 16), _source("cfg4s5", 16)]
    ds = [_fresh(S12, 1)["w"], _fresh(S5, 1)["w"]]
    bad = P.CplexWrapper(); bad.resetParameters(_dst_params("cfg4s5", 16, 1, "plain"))   # the timing bit: a filter outside 1 .. 15
    assert bad.setSolutionPool(16) == 0 and bad.setSolutionPoolFilter(16 | FILTER) == 0 and bad.callCplex() == P.OptimizationStatus.SUCCESS
    everyone = ds + [bad] + [s["w"] for s in srcs]
    before = [_pbytes(w) for w in everyone]
    assert all(b[0] >= 1 for b in before)
    out = (PoolCarryC * 32)()
    for o in out:
        o.status = 9
    counts = (C.c_int * 2)(7, 7)
    hs = (C.c_void_p * 2)(*[s["w"]._h for s in srcs])
    most = max(s["n"] for s in srcs)
    # a cap below the source entries of one pair
    assert L.miqp_solver_pool_carry_multi((C.c_void_p * 2)(ds[0]._h, ds[1]._h), hs, 2, 1, -1.0, out, most - 1, counts) == -2
    assert [o.status for o in out] == [9] * 32 and list(counts) == [7, 7] and [_pbytes(w) for w in everyone] == before
    # one pair under a filter outside 1 .. 15: it is named in ITS destination's last error
    assert L.miqp_solver_pool_carry_multi((C.c_void_p * 2)(ds[0]._h, bad._h), hs, 2, 1, -1.0, out, 16, counts) == -2
    assert "pair 1" in bad.lastError() and "filter %d" % (16 | FILTER) in bad.lastError() and ds[0].lastError() == ""
    with pytest.raises(RuntimeError, match=r"\(-2\).*pair 1"):
        P.carry_solution_pools([ds[0], bad], [s["w"] for s in srcs])
    assert [o.status for o in out] == [9] * 32 and list(counts) == [7, 7] and [_pbytes(w) for w in everyone] == before

"""Parity of the HIP solver (through the C ABI) with the CPU oracle and the reference's known answers.
All tests here need a real MI355X: run with  python -m pytest tests -m gpu."""
import os
import time

import numpy as np
import pytest

import planner_miqp_amd as P
from helpers import CONT_FIELDS, dat_path, k3, k3_results, load_params
from planner_miqp_amd import synthetic

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-4      # north_star: trajectory states within 1e-4
OBJ_TOL = 1e-5        # test/cplex_wrapper_test.cc:874 EXPECT_NEAR(..., 1e-5)


def gpu_solve_dat(name, gap):
    w = P.CplexWrapper("cplexmodel.mod", P.ParameterSource.DATFILE, 12, gap_override=gap)
    w.setParameterDatFileAbsolute(dat_path(name))
    st = w.callCplex()
    return w, st


def assert_regions_canonical_equal(p, a, b, tol=1e-5):
    """identical active regions, up to ties: where the labels differ the velocity must lie on the common border of
    the two sectors (both labels describe the same continuous point; SURVEY.md section 7, hard part 3)"""
    ra, rb = a.active_region.argmax(-1), b.active_region.argmax(-1)
    F = np.asarray(p.fraction_parameters, float).reshape(-1, 4)
    for c, i in np.argwhere(ra != rb):
        for res, j in ((a, rb[c, i]), (b, ra[c, i])):
            vx, vy = res.vel_x[c, i], res.vel_y[c, i]
            n1, n3 = np.hypot(F[j, 0], F[j, 1]), np.hypot(F[j, 2], F[j, 3])
            assert (F[j, 1] * vx - F[j, 0] * vy) / n1 <= tol and (F[j, 2] * vy - F[j, 3] * vx) / n3 <= tol, (c, i, ra[c, i], rb[c, i], vx, vy)


def assert_states_close(a, b, tol=STATE_TOL, fields=CONT_FIELDS):
    for n in fields:
        d = np.abs(getattr(a, n) - getattr(b, n)).max()
        assert d <= tol, (n, d)


def test_testcase_matches_reference_and_oracle(oracle):
    """test_problem_properties / test_hardcoded_data (cc:857-876): status 0, sizes, objective 9.57603 +- 1e-5;
    plus: bit-equal regions and states within 1e-4 of the CPU oracle, result feasible for the raw OPL rows"""
    w, st = gpu_solve_dat("cplexmodel_testcase.dat", 1e-6)
    assert st == P.OptimizationStatus.SUCCESS
    pr = w.getSolutionProperties()
    g = k3()
    assert abs(pr.objective - g["objective"]) <= OBJ_TOL
    assert (pr.NrConstraints, pr.NrBinaryVariables, pr.NrFloatVariables, pr.NonZeroCoefficients) == (12361, 1240, 340, 29834)   # cc:866-871
    assert pr.gap <= 1e-6 and pr.best_bound <= pr.objective + 1e-9 and pr.NrSolutionPool > 2   # cc:872-873: the incumbents found on the way
    assert pr.nodes >= 1 and pr.NrIterations >= pr.nodes and 0 < pr.time < 60   # search statistics are reported
    res = w.getRawResults()
    h = oracle.from_dat(dat_path("cplexmodel_testcase.dat"))
    ost, ores, op = oracle.solve(h, (1, 20, 32, 1, 1, 4), gap=1e-6)
    assert ost == 0 and abs(op.objective - pr.objective) <= 1e-6
    assert np.array_equal(res.active_region, ores.active_region)
    assert np.array_equal(res.active_region.reshape(-1), np.array(g["active_region"], dtype=np.int32))
    assert_states_close(res, ores)
    for n in ["deltacc", "deltacc_front", "notWithinEnvironmentRear", "region_change_not_allowed_combined"]:
        assert np.array_equal(getattr(res, n), getattr(ores, n)), n
    v, obj, worst = oracle.raw_eval(h, res)
    assert v < 1e-5 and abs(obj - pr.objective) < 1e-6, worst
    oracle.free(h)


def test_k3_fixed_binaries_on_device(oracle):
    """the device interior point kernel with K3's binaries asserted reproduces cc:283-456 and 9.57603"""
    fx, g = k3_results()
    w = P.CplexWrapper("cplexmodel.mod", P.ParameterSource.DATFILE, 12)
    w.setParameterDatFileAbsolute(dat_path("cplexmodel_testcase.dat"))
    rc, out, obj, it = w.solveFixed(fx)
    assert rc == 0 and abs(obj - g["objective"]) <= OBJ_TOL
    for n in CONT_FIELDS:
        ref = np.array(g[n]).reshape(1, 20)
        assert np.abs(getattr(out, n) - ref).max() <= 1e-4 + 5e-5 * np.abs(ref).max(), n
    h = oracle.from_dat(dat_path("cplexmodel_testcase.dat"))
    ost, ores, oobj, oit = oracle.solve_fixed(h, (1, 20, 32, 1, 1, 4), fx)
    assert ost == 0 and abs(oobj - obj) <= 1e-7
    assert_states_close(out, ores, 1e-5)
    oracle.free(h)


def test_hardcoded_data_versus_datfile():
    """cc:474-505: CPPINPUTS and DATFILE sources give the same objective and gap"""
    w1, st1 = gpu_solve_dat("cplexmodel_testcase.dat", 1e-6)
    w2 = P.CplexWrapper("cplexmodel.mod", P.ParameterSource.CPPINPUTS, 12, gap_override=1e-6)
    w2.resetParameters(load_params("cplexmodel_testcase.dat"))
    st2 = w2.callCplex()
    assert st1 == st2 == P.OptimizationStatus.SUCCESS
    assert abs(w1.getSolutionProperties().objective - w2.getSolutionProperties().objective) < 1e-9


def test_sos_and_priorities_do_not_change_the_answer(oracle):
    """cc:604-635, :755-791: SOS1 / branching priorities leave objective and gap unchanged"""
    objs = []
    for sos, prio in ((False, False), (True, False), (False, True)):
        w = P.CplexWrapper("cplexmodel.mod", P.ParameterSource.DATFILE, 12, gap_override=1e-5)
        w.setParameterDatFileAbsolute(dat_path("test_sos.dat"))
        w.setSpecialOrderedSets(sos); w.setUseBranchingPriorities(prio); w.setBranchingPriorityValueExtent(1, 19)
        assert w.callCplex() == P.OptimizationStatus.SUCCESS
        objs.append(w.getSolutionProperties().objective)
    assert max(objs) - min(objs) < 1e-9
    h = oracle.from_dat(dat_path("test_sos.dat"))
    ost, ores, op = oracle.solve(h, (1, 20, 16, 0, 0, 0), gap=1e-5)
    assert abs(op.objective - objs[0]) <= 2e-5 * abs(objs[0])
    oracle.free(h)


@pytest.mark.parametrize("cfg,seeds", [("mini1", range(6)), ("mini", range(6)), ("cfg2", range(4)), ("mini3", range(4)), ("mini4", range(3)),
                                       ("mini3b", range(4)), ("mini4b", range(4))])
def test_synthetic_parity_tight_gap(oracle, cfg, seeds):
    """seeded instances solved to 1e-7 by both: objective equal to 1e-6 relative, identical regions and
    canonical binaries, states within 1e-4, device result feasible for the raw big-M model"""
    for seed in seeds:
        p = synthetic.generate(cfg, seed, gap=1e-7, max_time=60)
        w = P.CplexWrapper(parameterSource=P.ParameterSource.CPPINPUTS)
        w.resetParameters(p)
        st = w.callCplex()
        h = oracle.from_params(p, 10)
        ost, ores, op = oracle.solve(h, oracle.dims(p), gap=1e-7, time_limit=120)
        assert int(st) == ost, (cfg, seed, st, ost)
        if ost != 0:
            oracle.free(h); continue
        pr = w.getSolutionProperties(); res = w.getRawResults()
        assert abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (cfg, seed, pr.objective, op.objective)
        assert_regions_canonical_equal(p, res, ores)
        assert_states_close(res, ores)
        for n in ["notWithinEnvironmentRear", "notWithinEnvironmentFrontUbUb", "deltacc", "deltacc_front", "car2car_collision",
                  "region_change_not_allowed_combined", "region_change_not_allowed_x_positive"]:
            assert np.array_equal(getattr(res, n), getattr(ores, n)), (cfg, seed, n)
        v, obj, worst = oracle.raw_eval(h, res)
        assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), (cfg, seed, worst)
        oracle.free(h)


LEAF_BINARIES = ["notWithinEnvironmentRear", "notWithinEnvironmentFrontUbUb", "deltacc", "deltacc_front", "car2car_collision",
                 "region_change_not_allowed_combined", "region_change_not_allowed_x_positive"]


def _oracle_many(oracle, ps, gap, limit, threads=48):
    from concurrent.futures import ThreadPoolExecutor

    def orc(p):
        h = oracle.from_params(p, 10)
        r = oracle.solve(h, oracle.dims(p), gap=gap, time_limit=limit)
        oracle.free(h)
        return r
    with ThreadPoolExecutor(min(threads, os.cpu_count() or 8)) as ex:
        return list(ex.map(orc, ps))


@pytest.mark.parametrize("cfg,seeds,need,gap,olimit", [("cfg3", range(700, 748), 30, 1e-7, 20), ("cfg4", range(1000, 1032), 14, 1e-7, 20),
                                                       ("cfg5s", [0, 1, 2, 3, 4, 5, 7, 9, 10, 12], 10, 1e-6, 60)])
def test_full_size_parity_at_a_tight_gap(oracle, cfg, seeds, need, gap, olimit):
    """the shape the bench times (2 cars x 20 steps x 32 regions; cfg4: + 4 moving obstacles) at gap 1e-7 on the seeds the CPU
    oracle proves within 20 s: objective equal to 1e-6 relative, identical regions (up to ties on a sector border), canonical leaf
    binaries equal, states within 1e-4, device result feasible for every raw big-M row - the bar of test/cplex_wrapper_test.cc:857-876
    (exact sizes, objective 1e-5) and of north_star (identical assignments, states within 1e-4) at full size.
    cfg5s: the FOUR-car shape (4 cars x 10 steps x 32 regions, the 2 x 2-tiled interior point kernel) at gap 1e-6 on the ten seeds the
    oracle proves in seconds (0.2 - 16 s on 8 cores) - regions, leaf binaries and states for four cars, not only an objective bracket"""
    ps = [synthetic.generate(cfg, s, gap=gap, max_time=60) for s in seeds]
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    sts = P.solve_batch(ws)
    res = _oracle_many(oracle, ps, gap, olimit)
    compared = ties = sites = retried = 0

    def compare(seed, p, r, pr, ores, op):
        """the comparisons of one instance; returns (ties, sites) or raises"""
        assert abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (cfg, seed, pr.objective, op.objective)
        assert_regions_canonical_equal(p, r, ores)
        assert_states_close(r, ores, fields=CONT_FIELDS[:8])
        # Where the velocity of a (car, step) lies exactly on the border of two sectors both labels describe the same state (checked
        # above) and the two sides may each report either; the front axle point is DEFINED through the label's polynomial
        # (cplexmodel/model_region_constraints.mod:56-69), so front points and the binaries on them are compared at the other steps
        tie = r.active_region.argmax(-1) != ores.active_region.argmax(-1)          # [car, step]
        for n in CONT_FIELDS[8:]:
            d = np.abs(getattr(r, n) - getattr(ores, n))[~tie]
            assert d.size == 0 or d.max() <= STATE_TOL, (cfg, seed, n, d.max())
        anystep = tie.any(0)                                                         # [step]
        for n in LEAF_BINARIES:
            a, b = getattr(r, n), getattr(ores, n)
            if n == "car2car_collision":
                ok = np.array_equal(a[:, :, ~anystep], b[:, :, ~anystep])
            elif a.ndim >= 3:                                                        # [car, piece | obstacle, step, ...]
                m = np.broadcast_to(tie[:, None, :].reshape(tie.shape[0], 1, tie.shape[1], *([1] * (a.ndim - 3))), a.shape)
                ok = np.array_equal(a[~m], b[~m])
            else:
                ok = np.array_equal(a[~tie], b[~tie])
            assert ok, (cfg, seed, n)
        h = oracle.from_params(p, 10)
        v, obj, worst = oracle.raw_eval(h, r)
        oracle.free(h)
        assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), (cfg, seed, worst)
        return int(tie.sum()), tie.size

    for seed, p, w, st, (ost, ores, op) in zip(seeds, ps, ws, sts, res):
        pr = w.getSolutionProperties()
        if ost != 0 or op.status not in (101, 102):
            if ost == 1 and op.status == 103:   # the oracle proves the instance infeasible: so must the device
                assert st == P.OptimizationStatus.FAILED_NO_SOLUT and pr.status == 103, (cfg, seed, int(st), pr.status)
            continue   # the oracle ran into its limit: no optimum to compare with
        assert int(st) == 0 and pr.status in (101, 102) and pr.gap <= gap + 1e-12, (cfg, seed, int(st), pr.status, pr.gap)   # what the CPU proves in 20 s the device proves in 60
        compared += 1
        try:
            t_, s_ = compare(seed, p, w.getRawResults(), pr, ores, op)
        except AssertionError:
            # Two leaves whose optima lie within the gap of each other (1e-7 of the objective: a sector change one step earlier or later at a
            # velocity of a few mm/s off the border) are BOTH right answers at that gap, and which one a search returns depends on its order.
            # Such an instance is decided at a gap a hundred times tighter, by both sides afresh: there the answers must agree.
            retried += 1
            p2 = synthetic.generate(cfg, seed, gap=gap * 1e-2, max_time=60)
            w2 = P.CplexWrapper(); w2.resetParameters(p2)
            st2 = w2.callCplex(); pr2 = w2.getSolutionProperties()
            assert int(st2) == 0 and pr2.status in (101, 102), (cfg, seed, int(st2), pr2.status)
            (ost2, ores2, op2), = _oracle_many(oracle, [p2], gap * 1e-2, 120, threads=1)
            assert ost2 == 0 and op2.status in (101, 102), (cfg, seed, "the oracle does not decide the tie within its limit")
            t_, s_ = compare(seed, p2, w2.getRawResults(), pr2, ores2, op2)
        ties += t_; sites += s_
    assert retried <= max(2, compared // 10), (retried, compared)   # (alternative optima within the gap are the exception)
    print("[count] full_size_parity", cfg, "compared", compared, "ties", ties, "of", sites, "decided at the tighter gap", retried)
    assert compared >= need, compared
    assert ties <= 0.02 * sites, (ties, sites)   # ties are the exception: at most 2 % of the (car, step) sites


def _translated(p, dx):
    """the same scenario at another place of the map: everything that is a position along x moves by dx"""
    import copy
    q = copy.deepcopy(p)
    q.IntitialState = np.array(p.IntitialState, float); q.IntitialState[:, 0] += dx
    q.x_ref = np.array(p.x_ref, float) + dx
    q.MultiEnvironmentConvexPolygon = [np.array(e, float) + np.array([dx, 0.0]) for e in p.MultiEnvironmentConvexPolygon]
    q.ObstacleConvexPolygon = [[np.array(e, float) + np.array([dx, 0.0]) for e in o] for o in p.ObstacleConvexPolygon]
    return q


def test_translated_copies_in_one_queue_keep_their_own_solutions(oracle):
    """two copies of a scenario, one moved 16 m along the road, in the same queue: same binaries, the same objective to the bits an
    incumbent key holds - each instance must still return ITS trajectory (the incumbent's solution is looked up among the batch slots
    of the instance, not among all slots with that key): feasible for its own raw model, and the pair exactly 16 m apart"""
    DX = 16.0
    ps = []
    for s in range(24):
        p = synthetic.generate("cfg3", s, gap=0.01, max_time=20)
        ps += [p, _translated(p, DX)]
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    sts = P.solve_batch(ws, inflight=len(ws))
    same_key = 0
    for k in range(0, len(ps), 2):
        rr = []
        for j in (k, k + 1):
            assert int(sts[j]) == 0, (j, int(sts[j]))
            pr = ws[j].getSolutionProperties(); r = ws[j].getRawResults()
            h = oracle.from_params(ps[j], 10)
            v, obj, worst = oracle.raw_eval(h, r)
            oracle.free(h)
            assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), (j, worst, obj, pr.objective)
            rr.append((pr, r))
        if abs(rr[0][0].objective - rr[1][0].objective) <= 1e-9 * abs(rr[0][0].objective):   # (the searches of the two may stop at different incumbents within the gap)
            same_key += 1
            assert np.abs(rr[1][1].pos_x - rr[0][1].pos_x - DX).max() <= 1e-5 and np.abs(rr[1][1].pos_y - rr[0][1].pos_y).max() <= 1e-5, k
    print("[count] translated_copies same_key", same_key)
    assert same_key >= 22, same_key   # (24 of 24 in every run so far; two may stop at different incumbents within the gap)


def test_local_search_changes_the_order_not_the_answer(monkeypatch):
    """the local search around new incumbents and the skeleton roots (MIQP_LNS) inject heuristic nodes; they never replace the
    tree: with and without them the same optimum is proven (gap 1e-4: objectives within the gap of each other, each bound below the
    other's objective), and on an instance whose tree is mostly incumbent-finding the search with them is the shorter one"""
    out = {}
    for mode in ("0", "45"):
        monkeypatch.setenv("MIQP_LNS", mode)
        for seed in (1913, 662, 20):
            w = P.CplexWrapper(); w.resetParameters(synthetic.generate("cfg3", seed, gap=1e-4 if seed == 20 else 1e-2, max_time=60))
            assert int(w.callCplex()) == 0
            pr = w.getSolutionProperties()
            assert pr.status in (101, 102), (mode, seed, pr.status)
            out[(mode, seed)] = (pr.objective, pr.best_bound, pr.nodes)
    for seed in (1913, 662, 20):
        (oa, ba, na), (ob, bb, nb) = out[("0", seed)], out[("45", seed)]
        tol = 1e-9 * max(1.0, abs(oa))
        assert ba <= ob + tol and bb <= oa + tol, (seed, oa, ba, ob, bb)
        g = 1e-4 if seed == 20 else 1e-2
        assert abs(oa - ob) <= g * max(abs(oa), abs(ob)) + tol, (seed, oa, ob)
    # (what the local search is worth on one pinned instance depends on the order of the search around it - 2.4 M -> 0.16 M nodes in round 4,
    # 215 k -> 135 k in round 5, 237 k -> 450 k with the active-set launches of round 6: a count for the record, with a wide margin; the
    # worth of the heuristic is measured on queues, profiles/r04_local_search_modes.txt)
    print("[count] local search, seed 1913: nodes without / with", out[("0", 1913)][2], out[("45", 1913)][2])
    assert out[("45", 1913)][2] < 4 * out[("0", 1913)][2], (out[("0", 1913)][2], out[("45", 1913)][2])


def test_active_set_launches_change_the_work_not_the_answer(monkeypatch):
    """round 6: the node relaxations of two cars are solved by the dual active-set launches (as_onchip.hip; MIQP_AS, default 1) instead of the
    interior point (MIQP_AS=0, the state of rounds 1-5).  Both are exact solvers of the same node QP: at gap 1e-7 the same optimum must be
    proven (objective 1e-7 relative - the polish of the incumbent is the interior point's in both), with the same regions and states, on
    single solves, and on a queue the same instances must be proven with objectives inside the gap of each other; the active-set launches
    must really have run (their node count is reported), and must really be off at 0"""
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MIQP_AS", mode)
        for seed in (2, 5, 15, 20, 23):
            w = P.CplexWrapper(); w.resetParameters(synthetic.generate("cfg3", seed, gap=1e-7, max_time=60))
            assert int(w.callCplex()) == 0
            pr = w.getSolutionProperties()
            assert pr.status in (101, 102) and pr.gap <= 1e-7 + 1e-12, (mode, seed, pr.status, pr.gap)
            tm = w.lastTiming()
            assert (tm["as_nodes"] > 0) == (mode == "1"), (mode, seed, tm["as_nodes"])
            if mode == "1":
                assert tm["as_nodes"] + tm["as_unfinished"] >= 0.5 * pr.nodes, (seed, tm["as_nodes"], pr.nodes)   # (the ordinary nodes and most of the large ones)
            res[(mode, seed)] = (pr.objective, w.getRawResults())
        ps = [synthetic.generate("cfg3", s, gap=1e-2, max_time=20) for s in range(900, 996)]
        ws = []
        for p in ps:
            w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
        sts = P.solve_batch(ws, inflight=32)
        res[(mode, "queue")] = [(int(st), w.getSolutionProperties().status, w.getSolutionProperties().objective, w.getSolutionProperties().best_bound) for w, st in zip(ws, sts)]
    p0 = synthetic.generate("cfg3", 2, gap=1e-7, max_time=60)
    for seed in (2, 5, 15, 20, 23):
        (oa, ra), (ob, rb) = res[("0", seed)], res[("1", seed)]
        assert abs(oa - ob) <= 1e-7 * max(1.0, abs(oa)), (seed, oa, ob)
        assert_regions_canonical_equal(p0, ra, rb)
        assert_states_close(ra, rb, fields=CONT_FIELDS[:8])
    for k, ((sa, ca, oa, ba), (sb, cb, ob, bb)) in enumerate(zip(res[("0", "queue")], res[("1", "queue")])):
        assert sa == 0 and sb == 0 and ca in (101, 102) and cb in (101, 102), (k, sa, ca, sb, cb)
        tol = 1e-9 * max(1.0, abs(oa))
        assert ba <= ob + tol and bb <= oa + tol and abs(oa - ob) <= 1e-2 * max(abs(oa), abs(ob)) + tol, (k, oa, ba, ob, bb)


def test_re_rounding_of_infeasible_probes_changes_the_order_not_the_answer(monkeypatch):
    """while an instance has no incumbent, an infeasible rounding probe is re-rounded from its least-violation solution (MIQP_PUMP
    generations, eval_kernel); like every heuristic node it never replaces the tree: with and without it the same optimum is proven, and
    the 4-car instance whose probes are ALL infeasible at first (cfg5 seed 2: 7.9 s without, 0.65 s with it) is proven inside 4 s only with it"""
    out = {}
    for mode in ("0", "6"):
        monkeypatch.setenv("MIQP_PUMP", mode)
        for cfg, seed, gap in (("cfg3", 20, 1e-4), ("cfg3", 11, 1e-2), ("cfg5s", 1, 1e-4), ("mini4", 3, 1e-6)):
            w = P.CplexWrapper(); w.resetParameters(synthetic.generate(cfg, seed, gap=gap, max_time=60))
            assert int(w.callCplex()) == 0
            pr = w.getSolutionProperties()
            assert pr.status in (101, 102), (mode, cfg, seed, pr.status)
            out[(mode, cfg, seed)] = (pr.objective, pr.best_bound, gap)
    for (mode, cfg, seed), (oa, ba, gap) in out.items():
        if mode != "0":
            continue
        ob, bb, _ = out[("6", cfg, seed)]
        tol = 1e-9 * max(1.0, abs(oa))
        assert ba <= ob + tol and bb <= oa + tol, (cfg, seed, oa, ba, ob, bb)
        assert abs(oa - ob) <= gap * max(abs(oa), abs(ob)) + tol, (cfg, seed, oa, ob)
    w = P.CplexWrapper(); w.resetParameters(synthetic.generate("cfg5", 2, gap=1e-2, max_time=4.0))   # (MIQP_PUMP is 6 here)
    assert int(w.callCplex()) == 0 and w.getSolutionProperties().status in (101, 102)
    monkeypatch.setenv("MIQP_PUMP", "0")
    w = P.CplexWrapper(); w.resetParameters(synthetic.generate("cfg5", 2, gap=1e-2, max_time=4.0))
    assert int(w.callCplex()) == 0 and w.getSolutionProperties().status in (107, 108)


def test_result_records_built_in_a_batch_equal_the_lazy_ones():
    """miqp_solver_materialize_results (collectRawResults for a whole batch on host threads) leaves in every handle exactly the
    record that miqp_solver_get_results computes on demand"""
    ps = [synthetic.generate("cfg3", s, gap=0.01, max_time=20) for s in range(12)]
    a, b = [], []
    for p in ps:
        for lst in (a, b):
            w = P.CplexWrapper(); w.resetParameters(p); lst.append(w)
    assert all(int(s) == 0 for s in P.solve_batch(a)) and all(int(s) == 0 for s in P.solve_batch(b))
    assert P.materialize_results(a) == len(a) and P.materialize_results(a) == 0   # built once
    for wa, wb in zip(a, b):
        ra, rb = wa.getRawResults(), wb.getRawResults()
        for n in CONT_FIELDS + LEAF_BINARIES + ["active_region", "slackvars", "notWithinEnvironmentFrontLbLb"]:
            assert np.array_equal(getattr(ra, n), getattr(rb, n)), n


def test_cfg5s_four_cars_against_the_oracle(oracle):
    """cfg5s (4 cars x 10 steps x 32 regions: the largest 4-car shape the CPU oracle proves in seconds; the 4-car interior point
    kernel with the 2x2-tiled stage algebra): at gap 1e-3 both prove their gap, the objectives agree within the two gaps, each
    side's bound lies below the other side's solution, and the device result is feasible for the raw big-M model"""
    G = 1e-3
    for seed in range(4):
        p = synthetic.generate("cfg5s", seed, gap=G, max_time=60)
        w = P.CplexWrapper(); w.resetParameters(p)
        assert int(w.callCplex()) == 0, seed
        pr = w.getSolutionProperties(); res = w.getRawResults()
        h = oracle.from_params(p, 10)
        ost, ores, op = oracle.solve(h, oracle.dims(p), gap=G, time_limit=120)
        assert ost == 0 and pr.status in (101, 102) and pr.gap <= G + 1e-12 and op.gap <= G + 1e-12, (seed, pr.status, pr.gap, op.gap)
        assert abs(pr.objective - op.objective) <= 2 * G * abs(op.objective), (seed, pr.objective, op.objective)
        assert pr.best_bound <= op.objective * (1 + 1e-9) and op.best_bound <= pr.objective * (1 + 1e-9), (seed, pr.best_bound, op.best_bound)
        v, obj, worst = oracle.raw_eval(h, res)
        assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), (seed, worst)
        oracle.free(h)


def test_what_a_stream_retires_at_its_limit_is_still_a_valid_answer(oracle):
    """round 5's review, item 6: on the driver's stream a few instances in a thousand end with the time-limit verdict (CPLEX status 107:
    `cplex.solve()` returned an incumbent, not a proof - src/cplex_wrapper.cpp:190-248 maps it to SUCCESS).  What such an instance
    returns must still be right: the incumbent feasible for every row of the raw big-M model and evaluated correctly, its best_bound
    below the optimum the CPU oracle proves and its objective not below it.  A queue with a limit short enough that a good number of
    its instances are retired unfinished (0.15 s each, 48 in flight)"""
    seeds = list(range(3300, 3396))
    ps = [synthetic.generate("cfg3", s, gap=1e-4, max_time=0.15) for s in seeds]
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    sts = P.solve_batch(ws, inflight=48)
    retired = [(s, p, w) for s, p, w, st in zip(seeds, ps, ws, sts) if int(st) == 0 and w.getSolutionProperties().status == 107]
    print("[count] retired at their limit with an incumbent:", len(retired), "of", len(seeds))
    assert len(retired) >= 8, len(retired)
    for p in ps:
        p.max_solution_time = 60.0
    for _, p, _ in retired:
        p.relative_mip_gap_tolerance = 1e-2
    res = _oracle_many(oracle, [p for _, p, _ in retired], 1e-2, 40)   # (these are the hard ones: whatever the oracle has after 40 s - an incumbent is an upper bound of the optimum, its best bound a lower one)
    compared = 0
    for (s, p, w), (ost, ores, op) in zip(retired, res):
        pr = w.getSolutionProperties()
        h = oracle.from_params(p, 10)
        v, obj, worst = oracle.raw_eval(h, w.getRawResults())
        oracle.free(h)
        assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), (s, worst, obj, pr.objective)
        assert pr.best_bound <= pr.objective + 1e-9 and pr.gap > 1e-4, (s, pr.best_bound, pr.objective, pr.gap)
        if ost == 0 and op.status in (101, 102, 107):
            compared += 1
            tol = 1e-7 * max(1.0, abs(op.objective))
            assert pr.best_bound <= op.objective + tol, (s, pr.best_bound, op.objective)      # what it had proven so far is true: below a feasible point's value
            assert pr.objective >= op.best_bound - tol, (s, pr.objective, op.best_bound)      # and its incumbent is not below what the oracle has proven
    print("[count] of those, compared with the oracle's incumbent and bound:", compared)
    assert compared >= 4, compared


def test_four_cars_on_the_64_region_tables_against_the_oracle(oracle):
    """round 5's review, item 6: beyond cfg5s (32 regions) nothing with four cars was compared with anything but itself.  Four cars x 10
    steps on the 64-REGION tables of BASELINE config 5 (common/parameter/fitting_polynomial_parameters.hpp:875-1281; cfg5 itself - 30
    steps - is beyond the CPU oracle): at gap 1e-4 on the seeds the oracle proves within its limit the objectives agree within the two
    gaps, each side's bound lies below the other's solution, the regions agree (up to ties on a sector border) and the states to 1e-3
    where they do, and the device result is feasible for the raw big-M model"""
    G = 1e-4
    cfg = (4, 10, 64, 2, 0)
    seeds = list(range(8))
    ps = [synthetic.generate(cfg, s, gap=G, max_time=60) for s in seeds]
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    sts = [w.callCplex() for w in ws]
    res = _oracle_many(oracle, ps, G, 90)
    compared = same_leaf = 0
    for s, p, w, st, (ost, ores, op) in zip(seeds, ps, ws, sts, res):
        pr = w.getSolutionProperties()
        assert int(st) == 0 and pr.status in (101, 102) and pr.gap <= G + 1e-12, (s, int(st), pr.status, pr.gap)
        h = oracle.from_params(p, 10)
        v, obj, worst = oracle.raw_eval(h, w.getRawResults())
        oracle.free(h)
        assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), (s, worst)
        if ost != 0 or op.status not in (101, 102) or op.gap > G + 1e-12:
            continue
        compared += 1
        assert abs(pr.objective - op.objective) <= 2 * G * abs(op.objective), (s, pr.objective, op.objective)
        assert pr.best_bound <= op.objective * (1 + 1e-9) and op.best_bound <= pr.objective * (1 + 1e-9), (s, pr.best_bound, op.best_bound)
        r = w.getRawResults()
        # the same leaf on both sides (regions equal up to ties on a sector border): then the same states.  Two leaves within the gap of each
        # other - with 64 sectors of 5.6 degrees a velocity a few mm/s off a border is common - are both right at this gap
        try:
            assert_regions_canonical_equal(p, r, ores)
        except AssertionError:
            continue
        same_leaf += 1
        assert_states_close(r, ores, tol=1e-3, fields=CONT_FIELDS[:8])
    print("[count] four cars x 64 regions compared with the oracle:", compared, "of", len(seeds), "- the same leaf on both sides:", same_leaf)
    assert compared >= 3 and same_leaf >= 1, (compared, same_leaf)


def test_three_car_reference_fixture_beats_the_recorded_cplex_point(oracle):
    """cplexmodel.dat (K5: 3 cars, 8 steps, 11 environment pieces; the reference's modelRun.txt point evaluates to
    741.22 in the raw model): the device result within 5 s is feasible for the raw big-M model and not worse"""
    p = load_params("cplexmodel.dat")
    p.max_solution_time = 5.0
    w = P.CplexWrapper(parameterSource=P.ParameterSource.CPPINPUTS)
    w.resetParameters(p)
    st = w.callCplex()
    assert int(st) == 0
    pr = w.getSolutionProperties(); res = w.getRawResults()
    h = oracle.from_dat(dat_path("cplexmodel.dat"))
    v, obj, worst = oracle.raw_eval(h, res, use_real_slack=True)
    oracle.free(h)
    assert v < 1e-5, worst
    assert abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj))
    assert pr.objective <= 741.2226


def test_debug_outputs_round_trip(tmp_path):
    """test_hardcoded_data_versus_datfile (test/cplex_wrapper_test.cc:474-505): the parameter file written by the debug
    output of a CPPINPUTS solve, read back as DATFILE, gives the same status, objective and gap; the solution print and the
    LP export are written next to it (src/cplex_wrapper.cpp:141-155, 212-219)"""
    p = load_params("cplexmodel_testcase.dat")
    p.relative_mip_gap_tolerance = 1e-3
    cw = P.CplexWrapper("cplexmodel.mod", P.ParameterSource.CPPINPUTS, 12)
    cw.resetParameters(p)
    cw.setDebugOutputFilePath(str(tmp_path)); cw.setDebugOutputFilePrefix("rt_"); cw.setDebugOutputPrint(True)
    assert int(cw.callCplex()) == 0
    datfile = cw.getDebugOutputParameterFilePath()
    assert datfile.endswith("rt_parameters_0.txt") and (tmp_path / "rt_lpexport_0.lp").exists() and (tmp_path / "rt_solution_0.txt").exists()
    cw2 = P.CplexWrapper("cplexmodel.mod", P.ParameterSource.DATFILE, 12)
    cw2.setParameterDatFileAbsolute(datfile)
    assert int(cw2.callCplex()) == 0
    a, b = cw.getSolutionProperties(), cw2.getSolutionProperties()
    # EXPECT_DOUBLE_EQ: within 4 units in the last place
    assert a.status == b.status and abs(a.objective - b.objective) <= 4 * np.spacing(abs(a.objective)) and abs(a.gap - b.gap) <= 4 * np.spacing(max(abs(a.gap), 1e-300))
    txt = open(tmp_path / "rt_solution_0.txt").read()
    assert "pos_x = [[" in txt and "active_region = [[[" in txt


def test_repeated_single_solves_are_bit_identical():
    """CPLEX's default parallel mode is deterministic (the reference's test_hardcoded_data_versus_datfile relies on it,
    test/cplex_wrapper_test.cc:474-505): the same instance solved again returns the same objective, gap and node count,
    bit for bit - ties of the node selection are broken by the nodes' own keys and evaluation prunes with the incumbent
    of the start of the round, not by the order concurrent workgroups finish in"""
    for p in (synthetic.generate("cfg3", 5, gap=0.01, max_time=10), synthetic.generate("cfg3", 11, gap=0.1, max_time=10)):
        seen = set()
        for _ in range(4):
            w = P.CplexWrapper(); w.resetParameters(p)
            assert int(w.callCplex()) == 0
            s = w.getSolutionProperties()
            seen.add((float(s.objective).hex(), float(s.gap).hex(), int(s.nodes), int(s.NrIterations)))
        assert len(seen) == 1, seen


def test_last_solution_warmstart_through_mst_file(tmp_path):
    """LAST_SOLUTION_WARMSTART (src/cplex_wrapper.cpp:128-138, 206-209): the solve writes an .mst, the next solve reads
    it as MIP start; the start is accepted as first incumbent (objective not worse, far fewer nodes)"""
    p = synthetic.generate("cfg3", 3, gap=0.01, max_time=10)
    w = P.CplexWrapper(); w.tmpWarmstartFile_ = str(tmp_path / "ws.mst")
    w.resetParameters(p); w.setLastSolutionWarmstart(); w.deleteLastSolutionWarmstartFile()
    assert int(w.callCplex()) == 0
    first = w.getSolutionProperties()
    assert os.path.exists(w.getTmpWarmstartFile()) and "<CPLEXSolution" in open(w.getTmpWarmstartFile()).read()
    w2 = P.CplexWrapper(); w2.tmpWarmstartFile_ = w.tmpWarmstartFile_
    w2.resetParameters(p); w2.setLastSolutionWarmstart()
    assert int(w2.callCplex()) == 0
    second = w2.getSolutionProperties()
    assert second.objective <= first.objective * (1 + 1e-9)
    assert second.NrSolutionPool >= 1
    w2.deleteLastSolutionWarmstartFile()
    assert not os.path.exists(w.getTmpWarmstartFile())


def test_plan_loop_and_receding_horizon_warmstart():
    """MiqpPlanner::Plan's region-combination loop and CalculateWarmstart (src/miqp_planner.cpp:633-766, 787-1051) on the
    device solver: plan, shift the solution by one step, move the cars to step 2 of the plan, plan again with the
    shifted start: the start is accepted and the warm solve agrees with a cold solve of the same instance"""
    import copy
    from planner_miqp_amd import planner_core as K
    p = synthetic.generate("cfg3", 4, gap=1e-4, max_time=20)
    expect_init = np.asarray(p.initial_region).copy()
    p.initial_region = np.zeros_like(expect_init)            # Plan derives it from the initial velocity
    w = P.CplexWrapper()
    ok, st = K.plan(w, p)
    assert ok and int(st) == 0 and np.array_equal(np.asarray(p.initial_region), expect_init)
    r1 = w.getRawResults(); o1 = w.getSolutionProperties().objective
    warm = K.calculate_warmstart(r1, p.ts, p.minimum_region_change_speed)
    p2 = copy.deepcopy(p)
    N = p.NumSteps
    for c in range(p.NumCars):
        p2.IntitialState[c] = [r1.pos_x[c, 1], r1.vel_x[c, 1], r1.acc_x[c, 1], r1.pos_y[c, 1], r1.vel_y[c, 1], r1.acc_y[c, 1]]
        for name in ("x_ref", "y_ref", "vx_ref", "vy_ref"):
            a = np.asarray(getattr(p, name), float)
            nxt = a[c, N - 1] + (a[c, N - 1] - a[c, N - 2])
            getattr(p2, name)[c] = np.concatenate([a[c, 1:], [nxt]])
    wc = P.CplexWrapper(); okc, stc = K.plan(wc, copy.deepcopy(p2))
    ww = P.CplexWrapper(); okw, stw = K.plan(ww, p2, warm, P.WarmstartType.RECEDING_HORIZON_WARMSTART)
    assert okc and okw
    oc, ow = wc.getSolutionProperties(), ww.getSolutionProperties()
    assert abs(oc.objective - ow.objective) <= 2e-4 * max(1.0, abs(oc.objective))
    assert ow.NrSolutionPool >= 1 and o1 > 0


def test_batch_equals_single_solves():
    ps = [synthetic.generate("mini", s, gap=1e-6, max_time=60) for s in range(12)]
    singles = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); assert w.callCplex() == P.OptimizationStatus.SUCCESS
        singles.append(w.getSolutionProperties().objective)
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    sts = P.solve_batch(ws)
    assert all(s == P.OptimizationStatus.SUCCESS for s in sts)
    for w, o in zip(ws, singles):
        assert abs(w.getSolutionProperties().objective - o) <= 1e-6 * max(1.0, abs(o))


def test_streaming_admission_equals_the_batch():
    """miqp_solver_solve_stream: a queue of 96 instances drained with 8 / 32 in flight proves what the one-batch call proves
    (same optimum within the two gaps, every instance to its gap), SolutionProperties.time is the time from the admission and
    stays below the instance's own limit"""
    G = 1e-3
    ps = [synthetic.generate("cfg3", s, gap=G, max_time=20) for s in range(600, 696)]

    def run(inflight):
        ws = []
        for p in ps:
            w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
        sts = P.solve_batch(ws, inflight=inflight)
        return ws, sts
    wa, sa = run(None)
    assert all(int(s) == 0 and w.getSolutionProperties().status in (101, 102) for w, s in zip(wa, sa))
    for infl in (8, 32):
        wb, sb = run(infl)
        for k, (a, b, st) in enumerate(zip(wa, wb, sb)):
            pa, pb = a.getSolutionProperties(), b.getSolutionProperties()
            assert int(st) == 0 and pb.status in (101, 102) and pb.gap <= G + 1e-12, (infl, k, pb.status, pb.gap)
            assert abs(pa.objective - pb.objective) <= 2 * G * max(1.0, abs(pa.objective)), (infl, k)
            assert pb.best_bound <= pa.objective * (1 + 1e-9) and pa.best_bound <= pb.objective * (1 + 1e-9), (infl, k)
            assert 0.0 <= pb.time < 20.3
        ra, rb = wa[5].getRawResults(), wb[5].getRawResults()
        assert np.abs(ra.pos_x - rb.pos_x).max() < 0.5   # (the same optimum up to the gap; lazily fetched result records)


def test_context_is_reused_between_queues_and_lanes_prove_the_same(monkeypatch):
    """(a) a second queue of another length on the same slots reuses the device context (no reallocation of the pools: the
    set-up of the second call is a small fraction of the first) and proves the same optima as a fresh solve; (b) MIQP_LANES=2:
    the queue dealt to two contexts that share the device proves every instance to its gap with the same optimum"""
    import time
    G = 1e-3
    ps = [synthetic.generate("cfg2", s, gap=G, max_time=20) for s in range(700, 700 + 640)]

    def run(lo, hi, inflight):
        ws = []
        for p in ps[lo:hi]:
            w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
        t = time.time(); sts = P.solve_batch(ws, inflight=inflight); dt = time.time() - t
        assert all(int(s) == 0 and w.getSolutionProperties().status in (101, 102) for w, s in zip(ws, sts))
        return ws, dt, ws[0].lastTiming()
    wa, _, _ = run(0, 520, 256)            # builds the context for 256 slots
    wb, _, tb = run(0, 640, 256)           # longer queue, same slots: reused
    wc, _, tc = run(100, 420, 256)         # shorter queue: reused
    assert not tb["context_built"] and not tc["context_built"] and tb["context_s"] < 0.05 and tc["context_s"] < 0.05, (tb, tc)
    for a, b in zip(wa, wb[:520]):
        pa, pb = a.getSolutionProperties(), b.getSolutionProperties()
        assert pa.objective == pb.objective and pa.nodes == pb.nodes   # the same instance on the same slots: the same solve, bit for bit
    for a, c in zip(wa[100:420], wc):
        assert abs(a.getSolutionProperties().objective - c.getSolutionProperties().objective) <= 2 * G * max(1.0, abs(a.getSolutionProperties().objective))
    monkeypatch.setenv("MIQP_LANES", "2")
    wl, _, _ = run(0, 640, 256)
    for b, l in zip(wb, wl):
        pb, pl = b.getSolutionProperties(), l.getSolutionProperties()
        assert pl.gap <= G + 1e-12 and abs(pb.objective - pl.objective) <= 2 * G * max(1.0, abs(pb.objective))
        assert pl.best_bound <= pb.objective * (1 + 1e-9) and pb.best_bound <= pl.objective * (1 + 1e-9)


def test_streaming_retires_an_instance_at_its_own_time_limit():
    """every instance of a queue has ITS OWN max_solution_time, counted from its admission: one that cannot finish (gap 1e-9,
    0.4 s) is retired - it reports its incumbent with status 107 - and its slot goes to the next one; the others are proven"""
    import time
    ps = [synthetic.generate("cfg3", s, gap=0.01, max_time=30) for s in range(40)]
    hard = synthetic.generate("cfg3", 3314, gap=1e-9, max_time=0.4)   # (38 M node relaxations at gap 1e-2: seed 307, used until round 5, is proven in 0.37 s since round 6)
    ps.insert(3, hard)
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    t = time.time(); sts = P.solve_batch(ws, inflight=4); dt = time.time() - t
    for k, (w, st) in enumerate(zip(ws, sts)):
        pr = w.getSolutionProperties()
        if k == 3:
            assert (int(st) == 0 and pr.status == 107) or (int(st) == 3 and pr.status == 108), (int(st), pr.status)
            assert pr.time < 0.4 + 0.3
        else:
            assert int(st) == 0 and pr.status in (101, 102), (k, int(st), pr.status)
    assert dt < 25.0


def test_bounds_at_the_bench_tolerance_are_valid(oracle):
    """gap 1e-2, i.e. the loosest node tolerance (qp_tol 1e-6) with the bound lifting on - the setting of the bench: the
    reported best_bound of every proven instance lies below the optimum the oracle proves at 1e-6 (a lift that overshoots
    because the node's multipliers are inexact would show here), the objective within the gap above it"""
    from concurrent.futures import ThreadPoolExecutor
    ps = [synthetic.generate("cfg3", s, gap=1e-2, max_time=20) for s in range(700, 748)]
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    sts = P.solve_batch(ws)

    def orc(p):
        h = oracle.from_params(p, 10)
        r = oracle.solve(h, oracle.dims(p), gap=1e-6, time_limit=20)
        oracle.free(h)
        return r
    with ThreadPoolExecutor(min(48, os.cpu_count() or 8)) as ex:
        res = list(ex.map(orc, ps))
    checked = 0; seen = []
    for k, (w, st, (ost, r, op)) in enumerate(zip(ws, sts, res)):
        pr = w.getSolutionProperties()
        assert int(st) == 0 and pr.status in (101, 102), k
        if ost != 0 or op.gap > 1e-6 + 1e-12:
            continue   # the oracle ran into its limit: no optimum to compare with
        checked += 1; seen.append(700 + k)
        tol = 1e-7 * max(1.0, abs(op.objective))
        assert pr.best_bound <= op.objective + tol, (k, pr.best_bound, op.objective)
        assert op.objective * (1 - 1e-6) - tol <= pr.objective <= op.objective * (1 + 1e-2) + tol, (k, pr.objective, op.objective)
    print("[count] bounds_at_the_bench_tolerance checked", checked, seen)
    # the seeds the oracle proves at 1e-6 within 5 s on eight cores (31 within its 20 s there, 35 on the GPU box's host) must all have been compared
    must = {702, 703, 704, 705, 706, 707, 708, 709, 710, 713, 714, 717, 719, 720, 726, 728, 729, 731, 733, 734, 735, 736, 737, 741, 744, 745, 746}
    print("[count] seeds the oracle usually proves in time that were not compared this time:", sorted(must - set(seen)))
    assert checked >= 24 and len(must - set(seen)) <= 6, (checked, sorted(must - set(seen)))   # (how many the host oracle finishes depends on the host: a margin, not the exact set)


def test_batch_multi_shards_over_the_visible_devices():
    """miqp_solver_solve_batch_multi: instance b -> device b mod G with one host thread per device; on a
    one-GPU box G = 1, with more devices every shard runs on its own device - the results do not depend on G"""
    import torch
    ps = [synthetic.generate("mini", s, gap=1e-6, max_time=60) for s in range(12)]
    ref = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ref.append(w)
    assert all(s == P.OptimizationStatus.SUCCESS for s in P.solve_batch(ref))
    for g in sorted({1, torch.cuda.device_count()}):
        ws = []
        for p in ps:
            w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
        sts = P.solve_batch(ws, gpus=g)
        assert all(s == P.OptimizationStatus.SUCCESS for s in sts)
        for w, r in zip(ws, ref):
            assert abs(w.getSolutionProperties().objective - r.getSolutionProperties().objective) <= 1e-6 * max(1.0, abs(r.getSolutionProperties().objective))


def test_two_threads_with_their_own_handles():
    """handles are independent (src/cplex_wrapper.hpp:61-275: one IloEnv per wrapper): two threads solving different
    shapes at the same time on the same device get the answers of the sequential run"""
    import threading
    jobs = [("mini", 0), ("mini3", 1), ("mini1", 2), ("mini", 3), ("mini4", 0), ("mini1", 1)]
    def solve(cfg, seed):
        w = P.CplexWrapper(); w.resetParameters(synthetic.generate(cfg, seed, gap=1e-6, max_time=60))
        assert w.callCplex() == P.OptimizationStatus.SUCCESS
        return w.getSolutionProperties().objective
    seq = [solve(c, s) for c, s in jobs]
    out = [None] * len(jobs)
    def worker(ids):
        for k in ids:
            out[k] = solve(*jobs[k])
    ts = [threading.Thread(target=worker, args=(range(t, len(jobs), 2),)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for a, b in zip(seq, out):
        assert b is not None and abs(a - b) <= 1e-9 * max(1.0, abs(a))


SPLIT_SCRIPT = r"""
import os, sys, json
sys.path.insert(0, %r)
import torch, torch.distributed as dist
import planner_miqp_amd as P
from planner_miqp_amd import synthetic, sharding
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
torch.cuda.set_device(r %% torch.cuda.device_count())
mode = sys.argv[1]
out = []
if mode == "rccl":
    sharding.init_rccl_comm(torch.cuda.current_device())
    assert P.load_library().miqp_comm_selftest(P.wrapper.EXCHANGE_FN(), None, 0, 0) == 0
ex = None if mode == "rccl" else sharding.torch_exchange()
for cfg, seed in (("mini", 1), ("mini3b", 2), ("cfg3", 3)):
    x = P.CplexWrapper(device=torch.cuda.current_device()); x.resetParameters(synthetic.generate(cfg, seed, gap=1e-6, max_time=60))
    st = sharding.split_solve(x, ex)
    pr = x.getSolutionProperties(); res = x.getRawResults()
    out.append(dict(cfg=cfg, seed=seed, status=int(st), objective=pr.objective, bound=pr.best_bound, nodes=int(pr.nodes), px=res.pos_x.tolist() if res is not None else None))
allo = [None] * w
dist.all_gather_object(allo, out)
if r == 0:
    print("SPLIT_JSON " + json.dumps(allo))
if mode == "rccl":
    P.load_library().miqp_comm_finalize()
dist.destroy_process_group()
"""


def _run_split(tmp_path, mode, nproc):
    import json, subprocess, sys, socket
    script = tmp_path / "split.py"
    script.write_text(SPLIT_SCRIPT % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % nproc, "--master-addr", "127.0.0.1",
                          "--master-port", str(port), str(script), mode], capture_output=True, text=True, env=env, timeout=900)
    line = [l for l in out.stdout.splitlines() if l.startswith("SPLIT_JSON ")]
    return (json.loads(line[0][len("SPLIT_JSON "):]) if line else None), out


def test_tree_split_over_two_ranks_matches_the_plain_solve(tmp_path):
    """C1: one instance, its tree split over two ranks (two processes; on a one-GPU box they share the device),
    incumbent / bound / stop exchanged once per round by all-reduce(min) over the torch.distributed group, solution broadcast
    by the owner: both ranks return the same status, objective and trajectory, and they are those of the unsplit solve"""
    res, out = _run_split(tmp_path, "torch", 2)
    assert res is not None, out.stdout[-2000:] + out.stderr[-2000:]
    for a, b in zip(res[0], res[1]):
        assert a["status"] == b["status"] == 0 and a["objective"] == b["objective"] and a["px"] == b["px"], (a["cfg"], a["objective"], b["objective"])
        w = P.CplexWrapper(); w.resetParameters(synthetic.generate(a["cfg"], a["seed"], gap=1e-6, max_time=60))
        assert int(w.callCplex()) == 0
        o = w.getSolutionProperties().objective
        assert abs(a["objective"] - o) <= 2e-6 * max(1.0, abs(o)), (a["cfg"], a["objective"], o)
        assert a["bound"] <= a["objective"] + 1e-9


def test_tree_split_over_rccl(tmp_path):
    """the same exchange over the library's RCCL communicator (ncclAllReduce(min, uint64) / ncclBroadcast): one rank per
    visible device (a one-GPU box runs the degenerate one-rank communicator - RCCL does not place two ranks on one device)"""
    import torch
    n = max(1, min(2, torch.cuda.device_count()))
    res, out = _run_split(tmp_path, "rccl", n)
    assert res is not None, out.stdout[-2000:] + out.stderr[-2000:]
    if torch.cuda.device_count() >= 2:
        # with two devices in sight the exchange must really have run between two RCCL ranks - never the degenerate communicator
        assert len(res) == 2, len(res)
        for a, b in zip(res[0], res[1]):
            assert a["status"] == b["status"] == 0 and a["objective"] == b["objective"] and a["px"] == b["px"], (a["cfg"], a["objective"], b["objective"])
    for rk in res:
        for a in rk:
            assert a["status"] == 0 and a["bound"] <= a["objective"] + 1e-9
    for a in res[0]:
        w = P.CplexWrapper(); w.resetParameters(synthetic.generate(a["cfg"], a["seed"], gap=1e-6, max_time=60))
        assert int(w.callCplex()) == 0
        o = w.getSolutionProperties().objective
        assert abs(a["objective"] - o) <= 2e-6 * max(1.0, abs(o))


def test_infeasible_instance_reports_no_solution():
    """initial pose outside the environment: CPLEX status 'infeasible' -> FAILED_NO_SOLUT, NaN objective (cpp:231-240)"""
    p = synthetic.generate("mini1", 0)
    p.IntitialState = p.IntitialState.copy(); p.IntitialState[0, 3] = 9.0
    w = P.CplexWrapper(); w.resetParameters(p)
    assert w.callCplex() == P.OptimizationStatus.FAILED_NO_SOLUT
    pr = w.getSolutionProperties()
    assert np.isnan(pr.objective) and np.isnan(pr.gap)


def test_soft_obstacle_can_be_ignored_at_its_price(oracle):
    """obstacle_is_soft (obstacle_environment_constraints.mod:85-91): a soft obstacle adds the alternative 'ignored' at
    WEIGHTS_SLACK_OBSTACLE per point; device and oracle agree on objective and on the slack binaries"""
    hits = 0
    for seed in range(6):
        p = synthetic.generate("mini1", seed, gap=1e-7, max_time=60)
        p.obstacle_is_soft = [1]
        p.WEIGHTS_SLACK_OBSTACLE = 0.5       # cheap enough that driving through can pay off
        cx, cy, hl, hw = float(p.IntitialState[0, 0]) + 9.0, -1.75, 3.4, 1.9    # static box on the reference path
        box = np.array([[cx - hl, cy - hw], [cx + hl, cy - hw], [cx + hl, cy + hw], [cx - hl, cy + hw]])
        p.ObstacleConvexPolygon = [[box.copy() for _ in range(p.NumSteps)]]
        w = P.CplexWrapper(); w.resetParameters(p)
        st = w.callCplex()
        h = oracle.from_params(p, 10)
        ost, ores, op = oracle.solve(h, oracle.dims(p), gap=1e-7, time_limit=120)
        assert int(st) == ost
        if ost == 0:
            pr = w.getSolutionProperties(); res = w.getRawResults()
            assert abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (seed, pr.objective, op.objective)
            assert np.array_equal(res.slackvarsObstacle, ores.slackvarsObstacle) and np.array_equal(res.slackvarsObstacle_front, ores.slackvarsObstacle_front)
            hits += int(res.slackvarsObstacle.sum() + res.slackvarsObstacle_front.sum() > 0)
            v, obj, worst = oracle.raw_eval(h, res)
            assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), worst
        oracle.free(h)
    assert hits >= 1, "no instance used the soft alternative: the test would not exercise it"


# Soft obstacles beyond one car: (shape, tweak_instance arguments, obstacle_is_soft, seed, the oracle's objective at gap 1e-7, points its optimum ignores) with
# WEIGHTS_SLACK_OBSTACLE = 0.5.  Two cars on the on-chip blocks and the active-set launches, three cars on the wide memory-backed kernel, two obstacles
# of which the first is soft (T[i_obssoft + o] per obstacle).  With the obstacle hard, (2, 8, 32, 1, 1) seed 2 and all three (3, 6, 32, 1, 1) instances are
# infeasible - the obstacle lies on a car's start - and (2, 10, 32, 1, 2) seed 2 costs 89.401584: there the soft alternative is taken because it pays.
# Seed 1 of each shape is left out: the oracle needs 19 s to half a minute, or does not prove it in 60 s.
SOFT_WHOLE = [((2, 8, 32, 1, 1), {"ahead": 12.0, "spacing": 6.0}, [1], 0, 155.092349, 0), ((2, 8, 32, 1, 1), {"ahead": 12.0, "spacing": 6.0}, [1], 2, 85.882742, 7),
              ((2, 8, 32, 1, 1), {"ahead": 12.0, "spacing": 6.0}, [1], 3, 115.318736, 0),
              ((3, 6, 32, 1, 1), {"ahead": 12.0, "spacing": 6.0}, [1], 0, 130.462010, 4), ((3, 6, 32, 1, 1), {"ahead": 12.0, "spacing": 6.0}, [1], 2, 112.870128, 9),
              ((3, 6, 32, 1, 1), {"ahead": 12.0, "spacing": 6.0}, [1], 3, 121.693527, 3),
              ((2, 10, 32, 1, 2), {"ahead": 14.0, "spacing": 6.0}, [1, 0], 0, 194.334923, 0), ((2, 10, 32, 1, 2), {"ahead": 14.0, "spacing": 6.0}, [1, 0], 2, 88.174413, 1),
              ((2, 10, 32, 1, 2), {"ahead": 14.0, "spacing": 6.0}, [1, 0], 3, 120.934907, 0)]


def _soft_whole_instance(shape, tweak, mask, seed):
    from helpers import tweak_instance
    p = synthetic.generate(shape, seed, gap=1e-7, max_time=60)
    tweak_instance(p, **tweak)
    p.obstacle_is_soft = list(mask)
    p.WEIGHTS_SLACK_OBSTACLE = 0.5
    return p


@pytest.mark.parametrize("shape,tweak,mask,seed,known,ignored", SOFT_WHOLE, ids=["%dx%dx%d-seed%d" % (s[0], s[1], s[4], seed) for s, _, _, seed, _, _ in SOFT_WHOLE])
def test_soft_obstacle_beyond_one_car(oracle, shape, tweak, mask, seed, known, ignored):
    """as test_soft_obstacle_can_be_ignored_at_its_price, with two and three cars and with a hard obstacle beside the soft one: the oracle's status,
    its objective within 1e-6 relative, its slack binaries; the record feasible for the raw big-M model at the returned objective and clean for
    certify(); on the two-car shapes the active-set launches ran.  The oracle's own answer is the recorded one, so the instance is the one
    the table was made for"""
    p = _soft_whole_instance(shape, tweak, mask, seed)
    w = P.CplexWrapper(); w.resetParameters(p)
    st = w.callCplex()
    h = oracle.from_params(p, 10)
    ost, ores, op = oracle.solve(h, oracle.dims(p), gap=1e-7, time_limit=120)
    npts = int(ores.slackvarsObstacle[:, :, 1:].sum() + ores.slackvarsObstacle_front[:, :, 1:].sum())   # (the table counts the decisions: steps >= 1)
    at0 = int(ores.slackvarsObstacle[:, :, 0].sum() + ores.slackvarsObstacle_front[:, :, 0].sum())
    pr = w.getSolutionProperties(); res = w.getRawResults()
    print("SOFTWHOLE %s seed %d: status %d oracle %d objective %.8f oracle %.8f points %d oracle %d + %d at step 0, nodes %d as_nodes %d" % (
        shape, seed, int(st), ost, pr.objective, op.objective, int(res.slackvarsObstacle.sum() + res.slackvarsObstacle_front.sum()), npts, at0, pr.nodes, w.lastTiming()["as_nodes"]))
    assert ost == 0 and abs(op.objective - known) <= 1e-6 * known and npts == ignored, (shape, seed, ost, op.objective, npts)
    # with three cars the obstacle lies on the third car's start: the constant step 0 ignores those points at their price, and the records say so -
    # both used to leave the slack entries of step 0 at 0, a record that breaks the raw model's cardinality row A7.card by 1
    assert (at0 > 0) == (shape[0] == 3), (shape, seed, at0)
    assert int(st) == ost
    assert abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (shape, seed, pr.objective, op.objective)
    assert np.array_equal(res.slackvarsObstacle, ores.slackvarsObstacle) and np.array_equal(res.slackvarsObstacle_front, ores.slackvarsObstacle_front)
    assert res.slackvarsObstacle[:, [o for o, m in enumerate(mask) if not m]].sum() == 0 and res.slackvarsObstacle_front[:, [o for o, m in enumerate(mask) if not m]].sum() == 0
    v, obj, worst = oracle.raw_eval(h, res)
    assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), worst
    cert = w.certify()
    assert cert.status == 0 and cert.max_violation < 1e-5 and abs(cert.objective - pr.objective) <= 1e-6 * max(1.0, abs(pr.objective)), cert
    if shape[0] == 2:
        assert P.has_active_set(2, shape[1]) == 1 and w.lastTiming()["as_nodes"] > 0, w.lastTiming()
    oracle.free(h)


def test_the_pool_calls_keep_the_price_of_ignored_points():
    """(2, 8, 32, 1, 1) seed 2, whose optimum ignores 7 points at 0.5 each (4 % of its objective), solved with a filtered pool of 8: the climb's
    tight-tolerance objective of every entry is the search's within the 0.1 % the node tolerance leaves (the search charges the price in
    eval_kernel, the pool calls in the collect kernels they share with solveFixedBatch); the explored entries and the refinement come out with
    objectives that certify() - the raw big-M model, which charges the weight itself - reproduces to 1e-9 relative; entry 0 is the solve's answer"""
    shape, tweak, mask, seed, known, ignored = SOFT_WHOLE[1]
    assert ignored > 0
    w = P.CplexWrapper(); w.resetParameters(_soft_whole_instance(shape, tweak, mask, seed))
    assert w.setSolutionPool(8) == 0 and w.setSolutionPoolFilter(P.POOL_BY_OBSTACLE | P.POOL_BY_CAR_CAR) == 0
    assert w.callCplex() == P.OptimizationStatus.SUCCESS
    objective = w.getSolutionProperties().objective
    found = w.solutionPoolFound()
    Cn, N, O, L = shape[0], shape[1], shape[4], 4
    f_obs = Cn * N + 5 * Cn * N
    with_L = [k for k in range(len(found)) if (w.solutionPoolFoundDecisions(k)[f_obs:f_obs + 5 * Cn * O * N] >= L).any()]
    print("SOFTPOOL found %s entries with ignored points %s" % (list(found), with_L))
    assert len(found) >= 1 and 0 in with_L and abs(found[0] - objective) <= 1e-6 * abs(objective)
    rc, before, after, moves, status = w.improveSolutionPool(8)
    assert rc >= 0 and len(before) == len(found)
    for k in range(len(found)):
        if status[k] == 0:
            assert abs(before[k] - found[k]) <= 1e-3 * abs(found[k]) and after[k] <= before[k], (k, before[k], found[k], after[k])
    assert status[0] == 0
    rc, added = w.exploreSolutionPool(4)
    assert rc >= 0
    st, obj, viol, it, route = w.solveSolutionPool()
    kept = w.solutionPoolFound()
    print("SOFTPOOL improved %s explored %d refined %s" % (list(after), rc, list(obj)))
    assert len(obj) >= 1 and st[0] == 0 and abs(obj[0] - objective) <= 1e-6 * abs(objective), (obj[0], objective)
    for k in range(len(obj)):
        if st[k] != 0:
            continue
        assert obj[k] <= kept[k] * (1 + 1e-3), (k, obj[k], kept[k])
        rcr, rec = w.solutionPoolRecord(k)
        cert = w.certify(rec)
        assert rcr == 0 and cert.status == 0 and cert.max_violation < 1e-5, (k, cert)
        assert abs(cert.objective - obj[k]) <= 1e-9 * max(1.0, abs(obj[k])), (k, cert.objective, obj[k])


def test_the_soft_instances_beyond_one_car_use_and_refuse_the_soft_alternative():
    """per shape the oracle's optimum ignores a point on at least one listed seed, and - on the two-car shapes - none on at least one (on the three-car
    shape every listed instance has to ignore some: the obstacle lies on the third car's start)"""
    for shape in {s for s, _, _, _, _, _ in SOFT_WHOLE}:
        pts = [n for s, _, _, _, _, n in SOFT_WHOLE if s == shape]
        assert any(n > 0 for n in pts) and (shape[0] == 3 or any(n == 0 for n in pts)), (shape, pts)


def test_rejected_inputs_fail_loudly():
    """sizes the device kernels do not take are refused with FAILED_SEG_FAULT (never approximated): 5 cars; a batch whose
    instances differ in shape; an instance whose initial region is not a possible region"""
    p5 = synthetic.generate((5, 6, 32, 1, 0), 0)
    w = P.CplexWrapper(); w.resetParameters(p5)
    assert w.callCplex() == P.OptimizationStatus.FAILED_SEG_FAULT
    a, b = synthetic.generate("mini", 0), synthetic.generate("mini3", 0)
    wa, wb = P.CplexWrapper(), P.CplexWrapper()
    wa.resetParameters(a); wb.resetParameters(b)
    assert all(s == P.OptimizationStatus.FAILED_SEG_FAULT for s in P.solve_batch([wa, wb]))
    assert P.solve_batch([wa])[0] == P.OptimizationStatus.SUCCESS          # the same solver object still works afterwards


def test_override_solver_settings():
    """overrideSolverSettingsDataSource (src/cplex_wrapper.cpp:893-896): only the solver knobs are taken over"""
    p = synthetic.generate("mini", 1, gap=0.5, max_time=30)
    q = synthetic.generate("mini", 2, gap=1e-6, max_time=7)
    w = P.CplexWrapper(); w.resetParameters(p)
    w.overrideSolverSettingsDataSource(q)
    assert p.relative_mip_gap_tolerance == 1e-6 and p.max_solution_time == 7
    assert int(w.callCplex()) == 0 and w.getSolutionProperties().gap <= 1e-6


def test_time_limit_is_honoured():
    """test_max_solution_time (cc:637-672): SolutionProperties.time < max_solution_time + 0.3 s for limits of 1.0, 0.5 and
    100 s (the reference's timeeps); a time-limited incumbent is a SUCCESS (status 107); wall time of the whole call, which
    includes model set-up like the reference's callCplex, stays within 0.5 s of that"""
    import time
    # (cfg5 - 4 cars x 30 steps x 64 regions - seed 11 at gap 1e-9 is far beyond a second: its proof at 1e-2 takes 3.6 M node relaxations
    # (seed 0, used here until round 5, is now proven at 1e-9 in 0.46 s); the first, untimed solve builds the device context of that shape,
    # as a planner's first call would)
    w0 = P.CplexWrapper(); w0.resetParameters(synthetic.generate("cfg5", 11, gap=1e-9, max_time=0.2)); w0.callCplex()
    for limit, cfg, seed, gap in ((1.0, "cfg5", 11, 1e-9), (0.5, "cfg5", 11, 1e-9), (100.0, "cfg3", 5, 1e-2)):
        p = synthetic.generate(cfg, seed, gap=gap, max_time=limit)
        w = P.CplexWrapper(); w.resetParameters(p)
        if cfg == "cfg3":
            w.callCplex()          # (context of this shape)
        t = time.time(); st = w.callCplex(); dt = time.time() - t
        pr = w.getSolutionProperties()
        assert pr.time < limit + 0.3, (limit, pr.time)
        assert dt < limit + 0.3 + 0.5, (limit, dt)
        assert (st == P.OptimizationStatus.SUCCESS and pr.status in (101, 102, 107)) or st == P.OptimizationStatus.FAILED_TIMEOUT
        if limit < 2:
            assert pr.status in (107, 108)          # gap 1e-9 cannot be proven in a second: the limit is what ended the solve


def test_shorter_time_limit_is_not_better():
    """test_overwrite_parameters (cc:821-842): with a shorter limit the objective is not better and the gap not smaller"""
    res = []
    for limit in (0.3, 3.0):
        p = synthetic.generate("cfg3", 118, gap=1e-6, max_time=limit)
        w = P.CplexWrapper(); w.resetParameters(p)
        assert int(w.callCplex()) in (0, 3)
        res.append(w.getSolutionProperties())
    if not (np.isnan(res[0].objective) or np.isnan(res[1].objective)):
        assert res[0].objective >= res[1].objective * (1 - 1e-9) and res[0].gap >= res[1].gap - 1e-12


def test_warmstart_is_accepted_as_incumbent():
    """test_complete_warmstart_receding_horizon (cc:715-753): a feasible start vector is taken as incumbent"""
    fx, g = k3_results()
    w = P.CplexWrapper("cplexmodel.mod", P.ParameterSource.DATFILE, 12, gap_override=1e-6)
    w.setParameterDatFileAbsolute(dat_path("cplexmodel_testcase.dat"))
    w.addRecedingHorizonWarmstart(fx)
    assert w.callCplex() == P.OptimizationStatus.SUCCESS
    assert abs(w.getSolutionProperties().objective - g["objective"]) <= OBJ_TOL


def test_mip_start_with_wrong_leaf_binaries_is_repaired_from_its_regions():
    """CPLEX repairs an infeasible MIP start (repairtries, cplexmodel.mod:8-21; effort MIPStartSolveMIP, src/cplex_wrapper.cpp:634):
    here the region binaries of a start form a second root whose rounding completes the rest.  A start whose car/car and
    environment binaries are scrambled (its own QP is infeasible) must neither be accepted as it is nor hurt: same optimum,
    an incumbent from the first rounds (the solve needs no more nodes than the cold one plus a handful)"""
    p = synthetic.generate("cfg3", 7, gap=1e-4, max_time=30)
    w = P.CplexWrapper(); w.resetParameters(p)
    assert int(w.callCplex()) == 0
    pr = w.getSolutionProperties(); res = w.getRawResults()
    import copy
    bad = copy.deepcopy(res)
    bad.car2car_collision[...] = 1
    bad.car2car_collision[..., 1::4] = 0          # "car 1 is ahead in x" asserted everywhere: false for these two cars
    bad.notWithinEnvironmentRear[...] = 1; bad.notWithinEnvironmentRear[:, 1, :] = 0   # everything in the far piece: false
    w2 = P.CplexWrapper(); w2.resetParameters(p); w2.addRecedingHorizonWarmstart(bad)
    assert int(w2.callCplex()) == 0
    pr2 = w2.getSolutionProperties()
    assert pr2.status in (101, 102) and abs(pr2.objective - pr.objective) <= 2e-4 * max(1.0, abs(pr.objective))
    assert pr2.best_bound <= pr.objective * (1 + 1e-9) and pr2.NrSolutionPool >= 1


@pytest.mark.parametrize("cfg", ["cfg3", "cfg4"])
def test_full_size_properties(oracle, cfg):
    """BASELINE configs at full size (2 cars x 20 steps x 32 regions [+ 4 obstacles]): size-independent
    properties - status, bound <= objective, gap definition, feasibility of the returned vector for every raw
    big-M row with the returned binaries, objective recomputed from the vector"""
    ps = [synthetic.generate(cfg, s, gap=0.01, max_time=20) for s in range(8)]
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    sts = P.solve_batch(ws)
    nsolved = 0
    for p, w, st in zip(ps, ws, sts):
        pr = w.getSolutionProperties()
        if st != P.OptimizationStatus.SUCCESS:
            assert st in (P.OptimizationStatus.FAILED_TIMEOUT, P.OptimizationStatus.FAILED_NO_SOLUT)
            continue
        assert pr.best_bound <= pr.objective + 1e-9
        assert abs(pr.gap - abs(pr.best_bound - pr.objective) / (1e-10 + abs(pr.objective))) < 1e-12
        assert pr.status in (101, 102, 107) and (pr.status == 107 or pr.gap <= 0.01 + 1e-12)
        nsolved += pr.status != 107
        h = oracle.from_params(p, 10)
        v, obj, worst = oracle.raw_eval(h, w.getRawResults())
        assert v < 1e-5, (cfg, worst)
        assert abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj))
        oracle.free(h)
    assert nsolved == len(ps), nsolved   # every one of these seeds is proven to the gap well inside the limit


def test_cfg4_batch_of_256_with_dynamic_obstacles(oracle):
    """BASELINE config 4 at its real batch size: 256 receding-horizon instances (2 cars x 20 steps x 32 regions + 4 dynamic
    obstacles, seeds 1000..1255) in one batch call; every returned vector is feasible for every raw big-M row with the
    returned binaries, objective recomputed from the vector, bound/gap/status consistent"""
    ps = [synthetic.generate("cfg4", 1000 + b, gap=0.01, max_time=8) for b in range(256)]
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    sts = P.solve_batch(ws)
    nsolved = nfeas = ninfeasible = 0
    for p, w, st in zip(ps, ws, sts):
        pr = w.getSolutionProperties()
        if st != P.OptimizationStatus.SUCCESS:
            # the only failure this batch may show is a PROVEN infeasibility (an obstacle on a car's start position), and the CPU oracle
            # must reach the same verdict
            assert st == P.OptimizationStatus.FAILED_NO_SOLUT and pr.status == 103, (int(st), pr.status)
            h = oracle.from_params(p, 10)
            ost, _, op = oracle.solve(h, oracle.dims(p), gap=0.01, time_limit=20)
            oracle.free(h)
            assert ost == 1 and op.status == 103, (ost, op.status)
            ninfeasible += 1
            continue
        nfeas += 1
        assert pr.best_bound <= pr.objective + 1e-9 and pr.status in (101, 102, 107) and (pr.status == 107 or pr.gap <= 0.01 + 1e-12)
        nsolved += pr.status != 107
        h = oracle.from_params(p, 10)
        v, obj, worst = oracle.raw_eval(h, w.getRawResults())
        oracle.free(h)
        assert v < 1e-5, worst
        assert abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj))
    print("[count] cfg4 nsolved", nsolved, "ninfeasible", ninfeasible)
    assert nsolved + ninfeasible == 256 and ninfeasible <= 8, (nfeas, nsolved, ninfeasible)   # every instance decided inside its limit: proven to the gap, or proven infeasible (251 + 5 measured; each infeasible verdict is confirmed by the oracle above)


def _many_alternatives_instance(seed, N=14, E=20, L=20):
    import math
    p = synthetic.generate((1, N, 32, E, 1, L), seed, gap=1e-7, max_time=60)
    cx, cy, hl, hw = float(p.IntitialState[0, 0]) + 12.0, -1.75, 3.4, 1.9       # a 20-gon on the reference path
    a = 2 * math.pi * (np.arange(L) + 0.5) / L
    poly = np.stack([cx + math.sqrt(2) * hl * np.cos(a), cy + math.sqrt(2) * hw * np.sin(a)], 1)
    p.ObstacleConvexPolygon = [[poly.copy() for _ in range(N)]]
    return p


def test_disjunctions_with_twenty_alternatives_match_the_oracle(oracle):
    """20 environment pieces and a 20-edge obstacle: every alternative of a disjunction becomes a child (none dropped);
    objective equal to 1e-6 relative, states within 1e-4, result feasible for the raw model"""
    for seed in range(4):
        p = _many_alternatives_instance(seed)
        w = P.CplexWrapper(); w.resetParameters(p)
        st = w.callCplex()
        h = oracle.from_params(p, 10)
        ost, ores, op = oracle.solve(h, oracle.dims(p), gap=1e-7, time_limit=120)
        assert int(st) == ost == 0, (seed, st, ost)
        pr = w.getSolutionProperties(); res = w.getRawResults()
        assert abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (seed, pr.objective, op.objective)
        assert_states_close(res, ores)
        v, obj, worst = oracle.raw_eval(h, res)
        assert v < 1e-5, (seed, worst)
        oracle.free(h)
    big = synthetic.generate((1, 6, 32, 63, 0), 0)            # more alternatives than one branching can create: refused
    w = P.CplexWrapper(); w.resetParameters(big)
    assert w.callCplex() == P.OptimizationStatus.FAILED_SEG_FAULT


def test_both_warmstart_strategies_apply_both_starts(tmp_path):
    """BOTH_WARMSTART_STRATEGIES (src/cplex_wrapper.cpp:121-138): the receding-horizon start AND the .mst of the last
    solution are registered; a useless receding-horizon record does not hide a good last-solution file"""
    p = synthetic.generate("cfg3", 3, gap=1e-4, max_time=10)
    w = P.CplexWrapper(); w.tmpWarmstartFile_ = str(tmp_path / "ws.mst")
    w.resetParameters(p); w.setLastSolutionWarmstart(); w.deleteLastSolutionWarmstartFile()
    assert int(w.callCplex()) == 0
    best = w.getSolutionProperties().objective
    from planner_miqp_amd.ctypes_types import RawResults
    junk = RawResults(2, 20, 32, 2, 0, 0)                    # every binary 9999999: fixes nothing
    for n in CONT_FIELDS:
        getattr(junk, n)[...] = 0.0
    w2 = P.CplexWrapper(); w2.tmpWarmstartFile_ = w.tmpWarmstartFile_
    q = synthetic.generate("cfg3", 3, gap=1e-4, max_time=0.05)    # so short that only the roots are solved
    w2.resetParameters(q)
    w2.addRecedingHorizonWarmstart(junk, P.WarmstartType.BOTH_WARMSTART_STRATEGIES)
    assert w2.doWarmstart_ == P.WarmstartType.BOTH_WARMSTART_STRATEGIES
    assert int(w2.callCplex()) == 0
    assert abs(w2.getSolutionProperties().objective - best) <= 1e-6 * abs(best)


def test_full_size_bounds_are_mutually_valid(oracle):
    """2 cars x 20 steps x 32 regions at gap 1e-3, instances both sides finish: every reported lower bound is below the
    other side's feasible objective (a bound that overstates is caught by the other solver's solution), objectives agree
    within the two gaps"""
    from concurrent.futures import ThreadPoolExecutor
    G = 1e-3
    ps = [synthetic.generate("cfg3", s, gap=G, max_time=12) for s in range(300, 348)]
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    sts = P.solve_batch(ws)

    def orc(p):
        h = oracle.from_params(p, 10)
        r = oracle.solve(h, oracle.dims(p), gap=G, time_limit=12)
        oracle.free(h)
        return r
    with ThreadPoolExecutor(min(48, os.cpu_count() or 8)) as ex:
        res = list(ex.map(orc, ps))
    both = 0; seen = []; dev_ok = []
    for k, (w, st, (ost, r, op)) in enumerate(zip(ws, sts, res)):
        pr = w.getSolutionProperties()
        if int(st) == 0 and pr.gap <= G + 1e-9:
            dev_ok.append(300 + k)
        if ost != 0 or op.gap > G + 1e-9 or int(st) != 0 or pr.gap > G + 1e-9:
            continue
        both += 1; seen.append(300 + k)
        tol = 1e-7 * max(1.0, abs(op.objective))
        assert pr.objective >= op.best_bound - tol and op.objective >= pr.best_bound - tol, (k, pr.objective, pr.best_bound, op.objective, op.best_bound)
        assert abs(pr.objective - op.objective) <= 2 * G * max(1.0, abs(op.objective))
    print("[count] full_size_bounds_are_mutually_valid both", both, seen, "device proven", len(dev_ok), dev_ok)
    assert len(dev_ok) == 48, len(dev_ok)   # the device proves every one of the 48 at 1e-3 inside 12 s
    must = {300, 301, 302, 303, 304, 305, 306, 309, 310, 312, 314, 317, 318, 322, 324, 326, 331, 332, 333, 334, 335, 338, 339, 340, 341, 342, 346, 347}   # the oracle: within 5 s on eight cores
    print("[count] seeds the oracle usually proves in time that were not compared this time:", sorted(must - set(seen)))
    assert both >= 24 and len(must - set(seen)) <= 6, (both, sorted(must - set(seen)))


def test_cfg5_four_cars_64_regions_with_warmstart(oracle):
    """BASELINE config 5 at its full size (4 cars x 30 steps x 64 regions; raw model 142 720 rows / 13 800 binaries):
    a time-limited solve returns a vector that is feasible for every raw big-M row; fed back as MIP start
    (variables_warmstart) the next solve starts from it and is not worse"""
    p = synthetic.generate("cfg5", 0, gap=0.01, max_time=10.0)
    h = oracle.from_params(p, 10)
    assert oracle.sizes(h)["rows"] == 142720 and oracle.sizes(h)["bin"] == 13800
    w = P.CplexWrapper(); w.resetParameters(p)
    st = w.callCplex()
    assert int(st) == 0
    pr = w.getSolutionProperties(); res = w.getRawResults()
    assert pr.status in (101, 102) and pr.gap <= 0.01 + 1e-12 and pr.best_bound <= pr.objective + 1e-9 and pr.nodes > 1000   # proven to the 1 % gap inside the reference's 10 s
    v, obj, worst = oracle.raw_eval(h, res)
    assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), worst
    w2 = P.CplexWrapper(); w2.resetParameters(p)
    w2.addRecedingHorizonWarmstart(res)
    assert int(w2.callCplex()) == 0
    pr2 = w2.getSolutionProperties()
    # (not worse up to the accuracy incumbents are compared at: the node relaxations are solved to 1e-6 relative - kernels.hip QP_TOL -, and the local
    # search may hand back a neighbouring leaf that was better by less than that before the final polish)
    assert pr2.objective <= pr.objective * (1 + 2e-6) and pr2.NrSolutionPool >= 1
    v2, obj2, worst2 = oracle.raw_eval(h, w2.getRawResults())
    assert v2 < 1e-5, worst2
    oracle.free(h)


def test_cfg5_all_sixteen_seeds_one_at_a_time(oracle):
    """BASELINE config 5 at its full size on all sixteen seeds 0..15, one callCplex each with the reference's 10 s limit and 1 % gap: at
    least 15 are proven to the gap (profiles/r04b_cfg5.txt: seed 11 is the one that can end at a gap of a few per cent), every returned vector -
    proven or time-limited - is feasible for every raw big-M row with the returned binaries, and no solve outlives its limit by more than
    the reference's own tolerance (test/cplex_wrapper_test.cc:644: limit + 0.3 s; here + 1 s for the result record of 13 800 binaries)"""
    proven = 0; left = []; t_proven = 0.0; nodes_left = []
    for seed in range(16):
        p = synthetic.generate("cfg5", seed, gap=0.01, max_time=10.0)
        w = P.CplexWrapper(); w.resetParameters(p)
        t = time.time(); st = w.callCplex(); dt = time.time() - t
        pr = w.getSolutionProperties()
        assert int(st) == 0 and pr.status in (101, 102, 107), (seed, int(st), pr.status)
        assert pr.time <= 10.0 + 1.0, (seed, pr.time, dt)
        if pr.status in (101, 102):
            assert pr.gap <= 0.01 + 1e-12, (seed, pr.gap)
            proven += 1; t_proven += pr.time
        else:
            left.append((seed, round(pr.gap, 4))); nodes_left.append(pr.nodes)
        h = oracle.from_params(p, 10)
        v, obj, worst = oracle.raw_eval(h, w.getRawResults())
        oracle.free(h)
        assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), (seed, worst)
    print("[count] cfg5 proven", proven, "of 16 in %.1f s of solve time; left at the limit:" % t_proven, left, "after", nodes_left, "node relaxations")
    assert proven >= 15, (proven, left)
    # the speed of the kernel of three and four cars (round 5: two wavefronts per node, sparse stage products, deferral of long nodes): the fifteen
    # take 7.8 s together (15.2 s with round 4's kernel), the sixteenth relaxes 2.5 M nodes in its 10 s (1.06 M)
    # (speed figures with a factor of two of margin - 7.8 s and 2.5 M measured: a shared or throttled device must not fail a parity suite)
    assert t_proven <= 24.0, t_proven
    assert all(nn >= 800_000 for nn in nodes_left), nodes_left


def test_single_solve_latency_of_the_planners_call_pattern():
    """one callCplex per instance on one reused wrapper, the way MiqpPlanner::Plan calls the path (src/miqp_planner.cpp:731), cfg3 seeds 0..95 at the
    reference's default gap 0.1: every solve proven, median <= 8 ms, 99 % quantile <= 55 ms, the slowest <= 75 ms (profiles/r05_single_latency.txt:
    4.9 / 46.6 / 58.4 ms on one MI355X; the reference's own tolerance is limit + 0.1 s, test/miqp_planner_test.cc:725)"""
    w = P.CplexWrapper(); lat = []
    for s in range(96):
        w.resetParameters(synthetic.generate("cfg3", s, gap=0.1, max_time=10.0))
        t = time.time(); st = w.callCplex(); dt = time.time() - t
        pr = w.getSolutionProperties()
        assert int(st) == 0 and pr.status in (101, 102), (s, int(st), pr.status)
        if s > 0:   # (the first call builds the device context)
            lat.append(dt)
    p50, p99, mx = (1e3 * float(np.percentile(lat, q)) for q in (50, 99, 100))
    print("[count] single solve latency ms p50 %.1f p99 %.1f max %.1f" % (p50, p99, mx))
    assert p50 <= 12.0 and p99 <= 100.0 and mx <= 150.0, (p50, p99, mx)   # (about twice what is measured: see the [count] line for the figures themselves)


def test_queue_node_counts_vary_little_between_runs():
    """a queue is not reproducible bit for bit (the order in which concurrent workgroups reserve batch slots and records moves the batch
    shares by a node or two: include/miqp_gpu.h) - but the spread is small and every verdict is the same: the same
    256-instance queue at 64 in flight three times: every instance proven each time, objectives within the gap of each other, total node
    relaxations within 2 % of each other"""
    ps = [synthetic.generate("cfg3", s, gap=0.01, max_time=20) for s in range(2000, 2256)]
    totals = []; objs = []
    for rep in range(3):
        ws = []
        for p in ps:
            w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
        sts = P.solve_batch(ws, inflight=64)
        prs = [w.getSolutionProperties() for w in ws]
        assert all(int(st) == 0 and pr.status in (101, 102) for st, pr in zip(sts, prs)), rep
        totals.append(sum(int(pr.nodes) for pr in prs)); objs.append([pr.objective for pr in prs])
    print("[count] queue node totals of three runs", totals)
    assert max(totals) <= 1.02 * min(totals), totals   # (identical totals in the runs so far: at 64 in flight every instance gets its whole share)
    for a, b in zip(objs[0], objs[2]):
        assert abs(a - b) <= 0.0101 * max(abs(a), abs(b)), (a, b)


def test_cut_gate_changes_the_work_not_the_answer(monkeypatch, oracle):
    """MIQP_CUT_GATE: the stationarity residual below which the early cutoff of a node relaxation is tested.  What is left of the residual
    enters the test (and the node's bound) with the instance's reachable-set diameter, so every gate is rigorous: with a loose gate (1e-2), the
    default (1e-5) and a tight one (1e-9) the same optima are proven to 1e-6, and each reported bound lies below the oracle's optimum"""
    seeds = (702, 705, 708, 713, 731, 746)
    ps = [synthetic.generate("cfg3", s, gap=1e-6, max_time=60) for s in seeds]
    ref = _oracle_many(oracle, ps, 1e-6, 40, threads=8)
    for gate in ("1e-2", "1e-5", "1e-9"):
        monkeypatch.setenv("MIQP_CUT_GATE", gate)
        for seed, p, (ost, ores, op) in zip(seeds, ps, ref):
            assert ost == 0 and op.gap <= 1e-6 + 1e-12, (seed, ost, op.gap)
            w = P.CplexWrapper(); w.resetParameters(p)
            assert int(w.callCplex()) == 0
            pr = w.getSolutionProperties()
            tol = 1e-7 * max(1.0, abs(op.objective))
            assert pr.status in (101, 102) and pr.gap <= 1e-6 + 1e-12, (gate, seed, pr.status, pr.gap)
            assert abs(pr.objective - op.objective) <= 2e-6 * abs(op.objective) + tol, (gate, seed, pr.objective, op.objective)
            assert pr.best_bound <= op.objective + tol, (gate, seed, pr.best_bound, op.objective)


@pytest.mark.parametrize("shape", [(1, 2, 16, 1, 0), (2, 2, 32, 1, 0), (2, 3, 16, 1, 0), (1, 40, 32, 1, 0), (1, 12, 32, 0, 0),
                                   (2, 6, 32, 0, 0), (2, 6, 16, 2, 1), (3, 4, 16, 1, 1)])
def test_odd_shapes_match_the_oracle(oracle, shape):
    """edge shapes: two- and three-step horizons, a 40-step horizon, no environment at all, 16 regions with two cars and an
    obstacle, three cars with an obstacle - objective equal to 1e-6 relative, states within 1e-4"""
    for seed in range(2):
        p = synthetic.generate(shape, seed, gap=1e-7, max_time=30)
        w = P.CplexWrapper(); w.resetParameters(p)
        st = w.callCplex()
        h = oracle.from_params(p, 10)
        ost, ores, op = oracle.solve(h, oracle.dims(p), gap=1e-7, time_limit=60)
        assert int(st) == ost, (shape, seed)
        if ost == 0:
            pr = w.getSolutionProperties(); res = w.getRawResults()
            assert abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (shape, seed, pr.objective, op.objective)
            assert_states_close(res, ores)
            v, obj, worst = oracle.raw_eval(h, res)
            assert v < 1e-5, (shape, seed, worst)
        oracle.free(h)


SEARCH_SCRIPT = r"""
import os, sys, json
sys.path.insert(0, %r)
import planner_miqp_amd as P
from planner_miqp_amd import synthetic
cap = int(sys.argv[1])
out = []
for cfg, seed, gap in (("cfg3", 0, 1e-6), ("cfg3", 2, 1e-6), ("cfg3", 5, 1e-6), ("cfg3", 33, 1e-4), ("cfg3", 118, 0.01), ("cfg4", 1, 1e-4)):
    w = P.CplexWrapper(max_open_nodes=cap); w.resetParameters(synthetic.generate(cfg, seed, gap=gap, max_time=60))
    st = w.callCplex(); pr = w.getSolutionProperties()
    out.append(dict(cfg=cfg, seed=seed, gap=gap, st=int(st), status=pr.status, objective=pr.objective, bound=pr.best_bound, nodes=int(pr.nodes)))
print("SEARCH_JSON " + json.dumps(out))
"""


def _run_search(tmp_path, cap, env_extra):
    import json, subprocess, sys
    script = tmp_path / "search.py"
    script.write_text(SEARCH_SCRIPT % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, str(script), str(cap)], capture_output=True, text=True, env=dict(os.environ, **env_extra), timeout=900)
    line = [l for l in out.stdout.splitlines() if l.startswith("SEARCH_JSON ")]
    assert line, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(line[0][len("SEARCH_JSON "):])


def test_search_devices_change_the_order_not_the_answer(tmp_path):
    """The two-tier open list and the bound lifting only reorder / prune the search: with the lifting switched off
    (MIQP_SEQ_KINDS bit 17), with the far tier switched off (MIQP_FAR_CAP=0) and with a near list of 65536 entries (a sixteenth of
    the default: the tiers spill and refill all the time), every instance is proven to its gap with the same optimum (own processes: the
    switches are read when the device context is built)."""
    ref = _run_search(tmp_path, 0, {})
    variants = {"no lifting": (0, {"MIQP_SEQ_KINDS": str((5 << 8) | 0x20000)}), "no far tier": (0, {"MIQP_FAR_CAP": "0"}),
                "short near list": (65536, {}),
                # near list of 2048 entries that the children fill to its capacity, far tier of 4 M entries: the refill takes its
                # threshold from a strided sample parked behind the list - which must stay inside the key array (round-2 advisor
                # finding: with n == cap the sample used to overwrite the keys of the next instance)
                "tiny near list, long far tier": (2048, {"MIQP_FAR_CAP": "4000000"}),
                "equal split of the batch (round-2 shares)": (0, {"MIQP_SEQ_KINDS": str((5 << 8) | 0x40000000)})}
    assert all(r["st"] == 0 and r["status"] in (101, 102) for r in ref), ref
    for name, (cap, env) in variants.items():
        got = _run_search(tmp_path, cap, env)
        for a, b in zip(ref, got):
            tol = max(2e-6, 2.0 * a["gap"]) * max(1.0, abs(a["objective"]))
            assert b["st"] == 0 and b["status"] in (101, 102), (name, b)
            assert abs(a["objective"] - b["objective"]) <= tol, (name, a, b)
            assert b["bound"] <= a["objective"] + tol and a["bound"] <= b["objective"] + tol, (name, a, b)
    # what the lifting buys on a hard instance (seed 118): fewer nodes (half of them at rounds of 4096 nodes, tools/seq_sweep.sh)
    nl = _run_search(tmp_path, 0, variants["no lifting"][1])
    assert ref[4]["nodes"] < nl[4]["nodes"], (ref[4]["nodes"], nl[4]["nodes"])


def test_c_api_known_answer_k8():
    """K8 (test/miqp_planner_c_api_test.cc:164-198, `get_raw_traj`): default settings, no map, one car starting at rest
    (0, vx 0, y 1, vy 0.01) on a straight reference line, desired velocity 5 reached 1 m ahead; AddCar -> Plan -> raw
    trajectory: time stamps 0 and 0.25, x(0) = 0 and x(0.25) = 0.005 +- 1e-3 (the car pulls away at the jerk limit)."""
    from planner_miqp_amd import planner_core as K
    pl = K.MiqpPlanner()
    idx = pl.AddCar([0, 0, 0, 1, 0.01, 0], [[0, 0], [5, 0], [30, 0]], 5, 1, 0.0, True)
    assert pl.Plan(0.0), pl.status
    N = pl.GetN()
    traj = pl.GetRawCMiqpTrajectory(idx, 0.0)
    assert traj.shape == (N, 9) and N == K.DefaultSettings()["nr_steps"]
    assert traj[0, 0] == 0 and traj[0, 1] == 0 and traj[1, 0] == 0.25
    assert abs(traj[1, 1] - 0.005) <= 1e-3, traj[:3]
    # the same model through the oracle: the device result is its optimum
    p = pl.GetParameters()
    assert abs(traj[1, 1] - traj[1, 7] * 0 - traj[0, 7] * 0.25 ** 3 / 6.0) < 1e-9      # x(0.25) = u_x(0) ts^3 / 6 from rest


def test_c_api_plan_with_a_dynamic_obstacle_and_after_removing_it():
    """`plan1` of the reference's C-API test (test/miqp_planner_c_api_test.cc:102-147): default settings, no map, the car of K8, an
    obstacle given by its four corner points per step (1 x 1 m at x = 10 .. 11 on the reference line, not static, hard):
    AddObstacle returns id 0, Plan succeeds with the obstacle and again after RemoveAllObstacles"""
    from planner_miqp_amd import planner_core as K
    pl = K.MiqpPlanner()
    pl.AddCar([0, 0, 0, 1, 0.01, 0], [[0, 0], [5, 0], [30, 0]], 5, 1, 0.0, True)
    N = pl.GetN()
    ob = [np.array([[10, -0.5], [11, -0.5], [11, 0.5], [10, 0.5]], float) for _ in range(N)]      # p1 .. p4 of the test, counter-clockwise
    assert pl.AddObstacle(ob, is_soft=False, is_static=False) == 0
    p = pl.GetParameters()
    assert p.nr_obstacles == 1 and p.max_lines_obstacles == 4
    assert pl.Plan(0.0), pl.status
    r = pl.GetSolution()
    # the rear axle point stays outside the box at every step (obstacle_environment_constraints.mod:52-96)
    inside = (r.pos_x[0] > 10 + 1e-6) & (r.pos_x[0] < 11 - 1e-6) & (np.abs(r.pos_y[0]) < 0.5 - 1e-6)
    assert not inside.any()
    pl.RemoveAllObstacles()
    assert p.nr_obstacles == 0
    assert pl.Plan(0.0), pl.status


def test_two_static_obstacles_are_passed_left_then_right():
    """testTwoStaticObstacles_matlab (test/miqp_planner_test.cc:561-611): DefaultTestSettings (= the mirror's defaults, gap 0.1), a
    straight road -10 .. 80 x +-4 m (given here as the convex piece the reference's map shrinking by the collision radius leaves:
    -9 .. 79 x +-3), the car at 10 m/s on the centre line, two 1 x 1 m static boxes at (20, -1.5) and (40, +1.5), inflated by the
    collision radius.  Expected: y(2.5 s) in (0, 0.3) - the first box is passed on the left -, y(4.75 s) in (-0.3, 0) - the
    second on the right -, x advances, Plan succeeds"""
    from planner_miqp_amd import planner_core as K
    pl = K.MiqpPlanner(mapPieces=[[[-9, -3], [79, -3], [79, 3], [-9, 3]]])
    idx = pl.AddCar([0, 10, 0, 0, 0.1, 0], [[0, 0], [100, 0]], 10, 1)
    box = [[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]]
    assert pl.AddStaticObstacle(box, (20.0, -1.5, 0.0)) == 0
    assert pl.AddStaticObstacle(box, (40.0, 1.5, 0.0)) == 1
    p = pl.GetParameters()
    assert p.nr_obstacles == 2
    assert pl.Plan(), pl.status
    assert p.nr_environments == 1
    traj = pl.GetRawCMiqpTrajectory(idx)
    y, x = traj[:, 2], traj[:, 1]
    assert 0 < y[10] < 0.3 and -0.3 < y[19] < 0 and x[19] > x[0], (y[10], y[19])


def test_planner_mirror_receding_horizon_two_cars():
    """planner_core.MiqpPlanner as MiqpPlanner is used (test/miqp_planner_test.cc:795-898 pattern): two cars on parallel
    straight lanes, plan, move every car to the second step of its plan, update, plan again with the receding-horizon start:
    every plan succeeds, the trajectories are dynamically consistent (triple integrator) and the second plan continues the
    first (positions of the overlap agree within what the moved reference allows)."""
    from planner_miqp_amd import planner_core as K
    S = dict(K.DefaultSettings(), warmstartType=P.WarmstartType.RECEDING_HORIZON_WARMSTART, nr_regions=32)
    pl = K.MiqpPlanner(S)
    lanes = ([[0, 0], [100, 0]], [[0, 3.5], [100, 3.5]])
    cars = [pl.AddCar([0, 5.0, 0, 0, 0.0, 0], lanes[0], 8.0, 10.0), pl.AddCar([4.0, 6.0, 0, 3.5, 0.0, 0], lanes[1], 6.0, 10.0)]
    ts = pl.GetTs()
    last = None
    for step in range(3):
        assert pl.Plan(step * ts), (step, pl.status)
        trajs = [pl.GetRawCMiqpTrajectory(c, step * ts) for c in cars]
        for t in trajs:   # x_{i+1} = x_i + ts v_i + ts^2/2 a_i + ts^3/6 u_i, per axis
            for (p_, v_, a_, u_) in ((1, 3, 5, 7), (2, 4, 6, 8)):
                pred = t[:-1, p_] + ts * t[:-1, v_] + ts * ts / 2 * t[:-1, a_] + ts ** 3 / 6 * t[:-1, u_]
                assert np.allclose(pred, t[1:, p_], atol=1e-6)
        if last is not None:
            for a, b in zip(last, trajs):
                assert np.allclose(a[1, 1:7], b[0, 1:7], atol=1e-9)            # the new start is the old second step
                assert np.abs(a[2:8, 1] - b[1:7, 1]).max() < 0.5                # and the plan goes on from there
        last = trajs
        for c, t in zip(cars, trajs):
            pl.UpdateCar(c, [t[1, 1], t[1, 3], t[1, 5], t[1, 2], t[1, 4], t[1, 6]], lanes[c], (step + 1) * ts)


def test_receding_horizon_through_the_bark_trajectory():
    """TEST(miqp_planner, receding_horizon) (test/miqp_planner_test.cc:310-360): a 100 x 100 m free square, one car at (0, 1) with
    velocity (4, -0.1) and a reference along y = 0 at 10 m/s; eight times: Plan, read the plan as GetBarkTrajectory (time, x, y,
    theta, v), move the car to its second row through CarStateToMiqpState with a = (v1 - v0) / dt, UpdateCar.  Expected as in the
    reference: every Plan succeeds, x grows, y falls towards the reference line, v grows.  DefaultTestSettings = the mirror's
    defaults with the obstacle region of interest switched on (test/miqp_planner_test.cc:65-68)."""
    from planner_miqp_amd import planner_core as K
    S = dict(K.DefaultSettings(), obstacle_roi_filter=True, obstacle_roi_behind_distance=10.0, obstacle_roi_front_distance=100.0, obstacle_roi_side_distance=15.0)
    pl = K.MiqpPlanner(S, mapPieces=[[[-50, -50], [50, -50], [50, 50], [-50, 50]]])
    ref = [[0, 0], [1000, 0]]
    st = np.array([0, 4, 0, 1, -0.1, 0], float)
    idx = pl.AddCar(st, ref, 10, 1)
    dt = pl.GetTs()
    x, y, v = [st[0]], [st[3]], [float(np.hypot(st[1], st[4]))]
    t = 0.0
    while t < 2.0:
        assert pl.Plan(), (t, pl.status)
        tr = pl.GetBarkTrajectory(idx, t)
        assert tr.shape[1] == 5 and tr.shape[0] == pl.GetN()              # the car is never slower than 0.7 m/s: nothing is cut off
        assert tr[0, 0] == np.float64(np.float32(t)) or abs(tr[0, 0] - t) < 1e-6
        raw = pl.GetRawCMiqpTrajectory(idx, t)
        np.testing.assert_allclose(tr[:, 1:3], raw[:, 1:3], atol=0)        # x, y of the raw read-out
        np.testing.assert_allclose(tr[:, 3], np.arctan2(raw[:, 4], raw[:, 3]), atol=1e-15)
        np.testing.assert_allclose(tr[:, 4], np.hypot(raw[:, 3], raw[:, 4]), atol=1e-12)
        x.append(tr[1, 1]); y.append(tr[1, 2]); v.append(tr[1, 4])
        a = (tr[1, 4] - tr[0, 4]) / dt
        pl.UpdateCar(idx, K.MiqpPlanner.CarStateToMiqpState(tr[1, 1], tr[1, 2], tr[1, 3], tr[1, 4], a).reshape(6), ref)
        t = float(np.float32(t) + np.float32(dt))                          # (the reference counts in float)
    assert x[0] < x[-1] and y[0] > y[-1] and v[0] < v[-1], (x, y, v)


def test_the_launch_split_of_a_round_is_in_use_and_the_leaves_of_the_local_search_start_warm():
    """round 6, second half: the larger launches of a round take their nodes from class lists, and the leaves of the local search start from the
    active set of the solve that found the incumbent - where an active-set launch found it; the incumbents of seeds 1913 and 662
    come from interior point nodes and their leaves start cold, at 58 - 74 steps.  On a hard instance (seed 307: ~250 k nodes, 1270 leaves) solved in a fresh process
    with MIQP_STATS=1 the statistics of the larger active-set block must show local-search leaves, and their average number of Goldfarb-Idnani steps
    must be that of a warm start (cold: 57 on this instance; warm: 12.5), the optimum the one the interior-point-only build proves"""
    import re, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import planner_miqp_amd as P; from planner_miqp_amd import synthetic; "
            "w = P.CplexWrapper(); w.resetParameters(synthetic.generate('cfg3', 307, gap=1e-2, max_time=30)); st = int(w.callCplex()); pr = w.getSolutionProperties(); "
            "print('RESULT', st, pr.status, repr(pr.objective), pr.nodes)") % root
    outs = {}
    for mode in ("1", "0"):
        env = dict(os.environ, MIQP_STATS="1", MIQP_AS=mode)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-600:]
        m = re.search(r"RESULT (\d+) (\d+) (\S+) (\d+)", out.stdout)
        assert m and int(m.group(1)) == 0 and int(m.group(2)) in (101, 102), out.stdout[-300:]
        outs[mode] = (float(m.group(3)), out.stderr)
    oa, err = outs["1"]; ob, _ = outs["0"]
    assert abs(oa - ob) <= 1e-2 * max(abs(oa), abs(ob)) + 1e-9, (oa, ob)
    m = re.search(r"in the larger block (\d+) nodes \(([0-9.]+) steps\), of them leaves of the local search (\d+) \(([0-9.]+) steps\)", err)
    assert m, err[-800:]
    big, leaves, lsteps = int(m.group(1)), int(m.group(3)), float(m.group(4))
    print("larger block: %d nodes, %d local-search leaves at %.1f steps" % (big, leaves, lsteps))
    assert big > 0 and leaves > 100, (big, leaves)
    assert lsteps < 30.0, lsteps   # (a cold leaf takes the size of its active set + 4 steps: 57 on average on this instance)


def test_bench_dump_outputs_are_the_same_in_two_runs(tmp_path):
    """`bench.py --dump-outputs` twice with the same arguments (each a fresh process): the same instances, every one of the last timed step
    proven and written, and the two runs write the same arrays (to rounding: the queue is drained as a stream of its own, which meets no
    decision of the wall clock); bound <= objective within the gap, one active region per car and step"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", "mini", "--batch", "8", "--queue-factor", "2", "--steps", "2", "--warmup", "1",
                            "--no-cpu", "--no-extras", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
        o = json.loads(lines[0])
        assert o["steps"] == 2 and o["ms_per_step"] > 0 and o["proven_share"] == 1.0 and o["config"]["instances_attempted"] == 32
        du = o["dumped_outputs"]
        assert du["instances"] == 16 and du["of"] == 16 and du["left_out"] == 0 and du["last_written_instance_ended_s"] < du["first_time_limit_could_run_out_s"]
        runs.append({f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))})
    a, b = runs
    assert sorted(a) == sorted(b) and list(a["seed"]) == list(range(32, 48))
    for x in (a, b):
        assert np.all(x["status"] == int(P.OptimizationStatus.SUCCESS)) and np.all(np.isin(x["solution_status"], (101, 102)))
        assert all(np.all(np.isfinite(v)) for v in x.values())
        assert np.all(x["best_bound"] <= x["objective"] + 1e-9) and np.all(x["gap"] <= 0.01 + 1e-12)
        assert np.all(x["active_region"].sum(-1) == 1)
    for n in a:
        assert np.allclose(a[n], b[n], rtol=1e-9, atol=1e-9), n


def test_bench_dump_outputs_leaves_out_the_large_trees(tmp_path, monkeypatch):
    """the instances whose tree went beyond the dump's node limit are not written: they are counted and named, the others keep their place"""
    import bench
    seeds = list(range(8))
    ws = []
    for sd in seeds:
        w = P.CplexWrapper(); w.resetParameters(synthetic.generate("mini", sd, gap=0.01)); ws.append(w)
    sts = P.solve_batch(ws, inflight=4)
    assert all(st == P.OptimizationStatus.SUCCESS for st in sts)
    nodes = [w.getSolutionProperties().nodes for w in ws]
    cut = sorted(nodes)[len(nodes) // 2]
    assert min(nodes) <= cut < max(nodes), nodes
    monkeypatch.setattr(bench, "DUMP_NODES", cut)
    du = bench.dump_outputs(str(tmp_path), P, ws, sts, seeds)
    keep = [k for k in range(8) if nodes[k] <= cut]
    assert du["of"] == 8 and du["instances"] == len(keep) and du["left_out"] == 8 - len(keep) and du["left_out_larger_than_nodes"] == cut
    assert sorted(du["left_out_seeds"]) == [k for k in range(8) if nodes[k] > cut]
    assert list(np.load(str(tmp_path / "instance.npy"))) == keep and list(np.load(str(tmp_path / "seed.npy"))) == keep
    obj = np.load(str(tmp_path / "objective.npy")); px = np.load(str(tmp_path / "pos_x.npy"))
    for j, k in enumerate(keep):
        assert obj[j] == ws[k].getSolutionProperties().objective and np.array_equal(px[j], ws[k].getRawResults().pos_x)

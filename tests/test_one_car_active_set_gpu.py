"""The dual active-set launches on one-car instances (as_onchip_kernel<1, ...>): the node relaxations of one car with up to 20 steps are
active-set solves started from the parent's active set, as those of two cars are; MIQP_AS=0 gives the interior point back, per call.
Both are exact solvers of the same node QP, so the work moves and the answer does not.  All tests need a real MI355X."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import planner_miqp_amd as P
from helpers import BIN_FIELDS, CONT_FIELDS, dat_path
from planner_miqp_amd import synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG1 = (1, 20, 32, 1, 1)      # the shape of the reference's fixture cplexmodel_testcase.dat: 32 regions, one environment, one obstacle
CFG2 = (1, 20, 16, 1, 0)      # synthetic.CONFIGS["cfg2"]
SEEDS = range(24)
LEAF_BINARIES = ["notWithinEnvironmentRear", "notWithinEnvironmentFrontUbUb", "deltacc", "deltacc_front",
                 "region_change_not_allowed_combined", "region_change_not_allowed_x_positive"]
RECORD_FIELDS = BIN_FIELDS + CONT_FIELDS + ["slackvarsObstacle", "slackvarsObstacle_front"]

CHILD = r"""
import pickle, sys
sys.path.insert(0, %r)
import planner_miqp_amd as P
from planner_miqp_amd import synthetic
jobs = pickle.load(open(sys.argv[1], "rb"))
out = []
for shape, seed, gap in jobs:
    w = P.CplexWrapper(); w.resetParameters(synthetic.generate(shape, seed, gap=gap, max_time=60))
    st = int(w.callCplex()); pr = w.getSolutionProperties(); tm = w.lastTiming()
    rec = None
    if st == 0:
        r = w.getRawResults(); rec = {n: getattr(r, n).copy() for n in %r}
    out.append(dict(st=st, status=pr.status, objective=pr.objective, bound=pr.best_bound, nodes=int(pr.nodes), iters=int(pr.NrIterations),
                    as_nodes=tm["as_nodes"], as_unfinished=tm["as_unfinished"], rec=rec))
pickle.dump(out, open(sys.argv[2], "wb"))
"""


def solve_in_child(tmp_path, jobs, env_extra, tag):
    """the jobs [(shape, seed, gap)] solved one after the other in a fresh process with `env_extra` set"""
    jf, of, sf = tmp_path / ("jobs_%s.pkl" % tag), tmp_path / ("out_%s.pkl" % tag), tmp_path / ("child_%s.py" % tag)
    pickle.dump(list(jobs), open(jf, "wb"))
    sf.write_text(CHILD % (ROOT, RECORD_FIELDS))
    env = dict(os.environ); env.update(env_extra)
    subprocess.run([sys.executable, str(sf), str(jf), str(of)], check=True, timeout=600, env=env)
    return pickle.load(open(of, "rb"))


def solve_here(shape, seed, gap, max_time=60):
    p = synthetic.generate(shape, seed, gap=gap, max_time=max_time)
    w = P.CplexWrapper(); w.resetParameters(p)
    st = int(w.callCplex())
    return p, w, st


def record_bytes(r):
    return b"".join(np.ascontiguousarray(getattr(r, n)).tobytes() for n in RECORD_FIELDS)


def regions_equal_up_to_ties(p, ra, va, rb, vb, tol=1e-5):
    """(test_gpu_parity.assert_regions_canonical_equal on arrays) where the labels differ the velocity lies on the common border of the sectors"""
    F = np.asarray(p.fraction_parameters, float).reshape(-1, 4)
    la, lb = ra.argmax(-1), rb.argmax(-1)
    for c, i in np.argwhere(la != lb):
        for (vx, vy), j in ((va, lb[c, i]), (vb, la[c, i])):
            n1, n3 = np.hypot(F[j, 0], F[j, 1]), np.hypot(F[j, 2], F[j, 3])
            assert (F[j, 1] * vx[c, i] - F[j, 0] * vy[c, i]) / n1 <= tol and (F[j, 2] * vy[c, i] - F[j, 3] * vx[c, i]) / n3 <= tol, (c, i, la[c, i], lb[c, i])


@pytest.fixture(scope="module")
def on_runs():
    """every seed of the two shapes at gap 1e-7 with the launches on, in this process: (params, wrapper, status, timing) by (shape, seed)"""
    runs = {}
    for shape in (CFG1, CFG2):
        for seed in SEEDS:
            p, w, st = solve_here(shape, seed, 1e-7)
            runs[(shape, seed)] = (p, w, st, w.lastTiming())
    return runs


def test_active_set_launches_move_the_work_of_one_car_not_the_answer(on_runs, tmp_path):
    """launches on against MIQP_AS=0 (a fresh process: the interior point of ipm_onchip_kernel<1, ...>): same status, objective within 1e-6
    relative, same regions (up to ties on a sector border), leaf binaries and states; the launches really ran, and really are off at 0"""
    jobs = [(shape, seed, 1e-7) for shape in (CFG1, CFG2) for seed in SEEDS]
    off = solve_in_child(tmp_path, jobs, {"MIQP_AS": "0"}, "as0")
    as_nodes = as_unf = nodes = 0
    for (shape, seed, _), o in zip(jobs, off):
        p, w, st, tm = on_runs[(shape, seed)]
        assert o["as_nodes"] == 0 and o["as_unfinished"] == 0, (shape, seed, o["as_nodes"])
        assert st == o["st"], (shape, seed, st, o["st"])
        if st != 0:
            continue
        pr = w.getSolutionProperties()
        assert pr.status in (101, 102) and o["status"] in (101, 102) and pr.gap <= 1e-7 + 1e-12, (shape, seed, pr.status, pr.gap)
        assert abs(pr.objective - o["objective"]) <= 1e-6 * max(1.0, abs(o["objective"])), (shape, seed, pr.objective, o["objective"])
        assert tm["as_nodes"] > 0, (shape, seed, tm)
        as_nodes += tm["as_nodes"]; as_unf += tm["as_unfinished"]; nodes += pr.nodes
        r = w.getRawResults(); q = o["rec"]
        regions_equal_up_to_ties(p, r.active_region, (r.vel_x, r.vel_y), q["active_region"], (q["vel_x"], q["vel_y"]))
        for n in CONT_FIELDS[:8]:
            assert np.abs(getattr(r, n) - q[n]).max() <= 1e-4, (shape, seed, n)
        for n in LEAF_BINARIES:
            assert np.array_equal(getattr(r, n), q[n]), (shape, seed, n)
    assert as_nodes >= 0.5 * nodes and as_unf < 0.1 * as_nodes, (as_nodes, as_unf, nodes)   # (the ordinary nodes and most of the large ones)


def test_one_car_active_set_results_match_the_oracle_and_certify(on_runs, oracle):
    """the same solves against the CPU oracle (objective 1e-6 relative, the record feasible for the raw big-M rows) and through certify()"""
    from concurrent.futures import ThreadPoolExecutor
    keys = sorted(on_runs)

    def orc(k):
        p = on_runs[k][0]
        h = oracle.from_params(p, 10)
        return h, oracle.solve(h, oracle.dims(p), gap=1e-7, time_limit=120)
    with ThreadPoolExecutor(min(16, os.cpu_count() or 8)) as ex:
        ors = list(ex.map(orc, keys))
    solved = 0
    for k, (h, (ost, ores, op)) in zip(keys, ors):
        p, w, st, tm = on_runs[k]
        assert st == ost, (k, st, ost)
        if ost == 0:
            pr = w.getSolutionProperties(); res = w.getRawResults()
            assert abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (k, pr.objective, op.objective)
            v, obj, worst = oracle.raw_eval(h, res)
            assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), (k, worst)
            cert = w.certify()
            assert cert.status == 0 and cert.max_violation < 1e-5 and cert.max_int_infeas == 0, (k, cert)
            assert abs(cert.objective - pr.objective) <= 1e-6 * max(1.0, abs(pr.objective)), (k, cert)
            solved += 1
        oracle.free(h)
    assert solved >= 40, solved


def test_reference_fixture_runs_on_the_active_set_launches():
    """cplexmodel_testcase.dat (test/cplex_wrapper_test.cc:857-876): 9.57603 and the raw sizes, now with active-set nodes"""
    w = P.CplexWrapper("cplexmodel.mod", P.ParameterSource.DATFILE, 12, gap_override=1e-6)
    w.setParameterDatFileAbsolute(dat_path("cplexmodel_testcase.dat"))
    assert w.callCplex() == P.OptimizationStatus.SUCCESS
    pr = w.getSolutionProperties()
    assert abs(pr.objective - 9.57603) <= 1e-5, pr.objective
    assert (pr.NrConstraints, pr.NrBinaryVariables, pr.NrFloatVariables, pr.NonZeroCoefficients) == (12361, 1240, 340, 29834)
    tm = w.lastTiming()
    assert tm["as_nodes"] > 0 and tm["as_steps"] >= tm["as_nodes"] and tm["std_launches"] > 0, tm
    assert w.certify().max_violation < 1e-5


def test_one_car_with_a_soft_obstacle_on_the_active_set_launches(oracle):
    """the instances of test_soft_obstacle_can_be_ignored_at_its_price (one car, ten steps, a cheap soft box on the reference path): the rows of a
    soft alternative carry a quadratic slack - the diagonal term 1 / a of the active-set method's Schur complement"""
    hits = 0
    for seed in range(6):
        p = synthetic.generate("mini1", seed, gap=1e-7, max_time=60)
        p.obstacle_is_soft = [1]
        p.WEIGHTS_SLACK_OBSTACLE = 0.5
        cx, cy, hl, hw = float(p.IntitialState[0, 0]) + 9.0, -1.75, 3.4, 1.9
        box = np.array([[cx - hl, cy - hw], [cx + hl, cy - hw], [cx + hl, cy + hw], [cx - hl, cy + hw]])
        p.ObstacleConvexPolygon = [[box.copy() for _ in range(p.NumSteps)]]
        w = P.CplexWrapper(); w.resetParameters(p)
        st = w.callCplex()
        h = oracle.from_params(p, 10)
        ost, ores, op = oracle.solve(h, oracle.dims(p), gap=1e-7, time_limit=120)
        assert int(st) == ost
        if ost == 0:
            pr = w.getSolutionProperties(); res = w.getRawResults()
            assert w.lastTiming()["as_nodes"] > 0, seed
            assert abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (seed, pr.objective, op.objective)
            assert np.array_equal(res.slackvarsObstacle, ores.slackvarsObstacle) and np.array_equal(res.slackvarsObstacle_front, ores.slackvarsObstacle_front)
            hits += int(res.slackvarsObstacle.sum() + res.slackvarsObstacle_front.sum() > 0)
            v, obj, worst = oracle.raw_eval(h, res)
            assert v < 1e-5 and abs(obj - pr.objective) <= 1e-6 * max(1.0, abs(obj)), worst
        oracle.free(h)
    assert hits >= 1, "no instance used the soft alternative: the test would not exercise it"


def test_repeated_one_car_solves_are_bit_identical(tmp_path):
    """the same instance five times in one process and once in a fresh one: identical result record, objective, bound and work"""
    for shape, seed, gap in ((CFG1, 3, 1e-4), (CFG2, 7, 1e-7)):
        seen = set()
        for _ in range(5):
            p, w, st = solve_here(shape, seed, gap)
            assert st == 0 and w.lastTiming()["as_nodes"] > 0
            s = w.getSolutionProperties()
            seen.add((float(s.objective).hex(), float(s.best_bound).hex(), int(s.nodes), int(s.NrIterations), record_bytes(w.getRawResults())))
        assert len(seen) == 1, [(a, b, c, d) for a, b, c, d, _ in seen]
        o = solve_in_child(tmp_path, [(shape, seed, gap)], {}, "rep%d" % seed)[0]
        rec = b"".join(np.ascontiguousarray(o["rec"][n]).tobytes() for n in RECORD_FIELDS)
        assert (float(o["objective"]).hex(), float(o["bound"]).hex(), o["nodes"], o["iters"], rec) in seen


@pytest.mark.parametrize("steps,launches", [(20, True), (21, False), (40, False)])
def test_the_dispatcher_draws_the_line_at_twenty_steps(oracle, steps, launches):
    """(1, 20, ...) has the launches, (1, 21, ...) and (1, 40, ...) - the memory-backed interior point - have not, as has_active_set says;
    all agree with the oracle"""
    assert P.has_active_set(1, steps) == int(launches)
    for seed in range(2):
        p, w, st = solve_here((1, steps, 32, 1, 0), seed, 1e-7, max_time=30)
        tm = w.lastTiming()
        assert (tm["as_nodes"] > 0) == launches and (launches or tm["as_nodes"] + tm["as_unfinished"] + tm["as_steps"] == 0), (steps, seed, tm)
        h = oracle.from_params(p, 10)
        ost, ores, op = oracle.solve(h, oracle.dims(p), gap=1e-7, time_limit=60)
        assert st == ost, (steps, seed)
        if ost == 0:
            pr = w.getSolutionProperties()
            assert abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (steps, seed, pr.objective, op.objective)
            v, obj, worst = oracle.raw_eval(h, w.getRawResults())
            assert v < 1e-5, (steps, seed, worst)
        oracle.free(h)


def test_one_car_queues_agree_with_single_solves():
    """a batch of one-car instances in one call, and as a stream with fewer slots than instances (the contexts' ring of inverses is reused
    across admissions): every instance proven to its gap, objectives within the gap of the single solves"""
    G = 1e-4
    jobs = [(CFG1, s) for s in range(100, 116)] + [(CFG2, s) for s in range(100, 116)]
    for shape in (CFG1, CFG2):
        ps = [synthetic.generate(sh, s, gap=G, max_time=30) for sh, s in jobs if sh == shape]
        singles = []
        for p in ps:
            w = P.CplexWrapper(); w.resetParameters(p); assert int(w.callCplex()) == 0
            singles.append(w.getSolutionProperties())
        for inflight in (None, 4):
            ws = []
            for p in ps:
                w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
            sts = P.solve_batch(ws, inflight=inflight)
            assert ws[0].lastTiming()["as_nodes"] > 0, (shape, inflight)
            for k, (w, st, a) in enumerate(zip(ws, sts, singles)):
                b = w.getSolutionProperties()
                assert int(st) == 0 and b.status in (101, 102) and b.gap <= G + 1e-12, (shape, inflight, k, b.status, b.gap)
                assert abs(a.objective - b.objective) <= 2 * G * max(1.0, abs(a.objective)), (shape, inflight, k, a.objective, b.objective)
                assert b.best_bound <= a.objective * (1 + 1e-9) + 1e-9 and a.best_bound <= b.objective * (1 + 1e-9) + 1e-9, (shape, inflight, k)
            cs = P.certify_batch(ws)
            assert max(c.max_violation for c in cs) < 1e-5


def test_two_cars_still_run_on_the_shared_kernel(oracle):
    """one cfg3 seed: the counters of the launches are there and the optimum is the oracle's (that the two-car code is the same instruction for
    instruction is shown by the compiler's output, not here)"""
    p, w, st = solve_here("cfg3", 5, 1e-7)
    assert st == 0
    tm = w.lastTiming(); pr = w.getSolutionProperties()
    assert tm["as_nodes"] > 0 and tm["as_nodes"] + tm["as_unfinished"] >= 0.5 * pr.nodes and tm["std_launches"] > 0, tm
    h = oracle.from_params(p, 10)
    ost, ores, op = oracle.solve(h, oracle.dims(p), gap=1e-7, time_limit=120)
    assert ost == 0 and abs(pr.objective - op.objective) <= 1e-6 * max(1.0, abs(op.objective)), (pr.objective, op.objective)
    oracle.free(h)

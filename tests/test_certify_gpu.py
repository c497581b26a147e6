"""Certificates computed on the device, each compared with the CPU oracle's raw-model evaluation of the same record."""
import copy
import ctypes as C

import numpy as np
import pytest

import planner_miqp_amd as P
from helpers import dat_path, k3_results
from planner_miqp_amd import synthetic

pytestmark = pytest.mark.gpu


def _dims(p):
    return (p.NumCars, p.NumSteps, p.nr_regions, p.nr_environments, p.nr_obstacles, p.max_lines_obstacles)


def _solve(p):
    w = P.CplexWrapper()
    w.resetParameters(p)
    assert w.callCplex() == P.OptimizationStatus.SUCCESS
    return w


def _check(oracle, h, cert, rec, real=True, tol=1e-9):
    v, obj, worst = oracle.raw_eval(h, rec, use_real_slack=real)
    assert cert.status == 0
    assert abs(cert.max_violation - v) <= tol * max(1.0, abs(v)), (cert, v, worst)
    assert abs(cert.objective - obj) <= 1e-9 * max(1.0, abs(obj)), (cert, obj)
    assert cert.family_violation.max() == cert.max_violation
    if cert.max_violation > 0:
        assert cert.worst_family == int(np.argmax(cert.family_violation)) + 1
        if v > 1e-6:      # (below that the worst row is decided by the last bits of two summation orders)
            assert cert.worst_row == int(worst.split("#")[1]), (cert, worst)
    else:
        assert cert.worst_family == 0 and cert.worst_row == -1
    return v, obj


def test_the_references_own_answer_certifies(oracle):
    dat = dat_path("cplexmodel_testcase.dat")
    w = P.CplexWrapper(parameterSource=P.ParameterSource.DATFILE)
    w.setParameterDatFileAbsolute(dat)
    r, _ = k3_results()
    cert = w.certify(r)
    h = oracle.from_dat(dat)
    v, obj = _check(oracle, h, cert, r)
    oracle.free(h)
    assert cert.rows == 12361 == w.rawSizes()["rows"]
    assert abs(cert.objective - 9.57603) < 5e-4      # K3 is the solution vector as the reference's test prints it (6 digits): 9.575839
    assert cert.max_int_infeas == 0.0


@pytest.mark.parametrize("cfg,seeds", [("mini", [0]), ("mini1", [0]), ("mini3", [0]), ("mini4", [0]), ("cfg3", range(8)), ("cfg4", range(4)),
                                       ((4, 10, 64, 2, 0), [0])])
def test_own_solutions_certify(oracle, cfg, seeds):
    for seed in seeds:
        p = synthetic.generate(cfg, seed, gap=1e-4)
        if cfg == "mini1":
            p.obstacle_is_soft = [1]
        w = _solve(p)
        cert = w.certify()
        h = oracle.from_params(p)
        rec = w.getRawResults()
        _check(oracle, h, cert, rec)
        assert cert.max_violation < 1e-5, (cfg, seed, cert)
        assert cert.rows == w.rawSizes()["rows"] and cert.max_int_infeas == 0.0
        assert w.certify(rec).raw == cert.raw          # the fetched record is the record the handle certified
        _check(oracle, h, w.certify(rec, use_real_slack=False), rec, real=False)
        oracle.free(h)


def _perturbed(oracle, w, h, rec, change, family, only=True):
    r2 = copy.deepcopy(rec)
    change(r2)
    cert = w.certify(r2)
    _check(oracle, h, cert, r2)
    if family is not None:
        assert cert.family_violation[family - 1] > 1e-3, cert
        if only:
            assert cert.worst_family == family, cert
    return cert


def test_it_sees_what_is_wrong(oracle):
    p = synthetic.generate("cfg3", 1, gap=1e-4)
    w = _solve(p); rec = w.getRawResults(); h = oracle.from_params(p)
    base = w.certify()
    assert base.max_violation < 1e-5

    def add_pos(r): r.pos_x[1, 7] += 0.5
    c = _perturbed(oracle, w, h, rec, add_pos, 2, only=False)
    assert abs(c.family_violation[1] - 0.5) < 1e-5

    def move_region(r):
        j = int(np.argmax(r.active_region[0, 5])); r.active_region[0, 5, :] = 0; r.active_region[0, 5, (j + 16) % 32] = 1
    _perturbed(oracle, w, h, rec, move_region, 4, only=False)

    def vx_high(r): r.vel_x[0, 3] = p.max_vel_x_y + 1.0
    c = _perturbed(oracle, w, h, rec, vx_high, 3, only=False)
    assert abs(c.family_violation[2] - 1.0) < 1e-6

    def vy_high(r): r.vel_y[0, 3] = p.max_vel_x_y + 1.0
    c = _perturbed(oracle, w, h, rec, vy_high, None)
    assert c.family_violation[2] == base.family_violation[2]      # the raw model bounds vel_x twice and vel_y never

    outside = np.argwhere(rec.notWithinEnvironmentRear == 1)
    assert len(outside), "cfg3 has two environment pieces: every car is outside of one of them somewhere"
    ci, e, i = outside[0]

    def clear_flag(r): r.notWithinEnvironmentRear[ci, e, i] = 0
    _perturbed(oracle, w, h, rec, clear_flag, 6)

    def int_two(r): r.active_region[1, 2, 0] = 2
    c = _perturbed(oracle, w, h, rec, int_two, None)
    assert c.max_int_infeas == 1.0
    oracle.free(h)

    p4 = synthetic.generate("cfg4", 0, gap=1e-4)
    w4 = _solve(p4); rec4 = w4.getRawResults(); h4 = oracle.from_params(p4)
    passed = np.argwhere(rec4.deltacc == 0)
    assert len(passed)
    q = tuple(passed[len(passed) // 2])

    def flip(r): r.deltacc[q] = 1 - r.deltacc[q]
    c = _perturbed(oracle, w4, h4, rec4, flip, None)
    ones = np.argwhere(rec4.deltacc == 1)
    hit = False
    for q1 in ones[:: max(1, len(ones) // 40)]:      # a set flag asserts the car beyond that edge: cleared, its row binds
        def clear(r, q1=tuple(q1)): r.deltacc[q1] = 0
        c = _perturbed(oracle, w4, h4, rec4, clear, None)
        if c.family_violation[6] > 1e-3:
            assert c.worst_family == 7
            hit = True
            break
    assert hit
    oracle.free(h4)

    pm = synthetic.generate("mini", 0, gap=1e-4)
    wm = _solve(pm); recm = wm.getRawResults(); hm = oracle.from_params(pm)

    def all_set(r): r.car2car_collision[0, 0, 3, :] = 1
    _perturbed(oracle, wm, hm, recm, all_set, 8)
    oracle.free(hm)


def test_int_and_real_slack_differ_as_the_oracles_modes_do(oracle):
    found = None
    for safety in (2.0, 1.0, 3.0):
        for seed in range(6):
            p = synthetic.generate("mini", seed, gap=1e-4)
            p.agent_safety_distance = np.full(p.NumSteps, safety)     # a soft distance the merging cars pay slack for
            w = P.CplexWrapper(); w.resetParameters(p)
            if w.callCplex() != P.OptimizationStatus.SUCCESS:
                continue
            rec = w.getRawResults()
            if np.abs(rec.slackvars_real).max() > 1e-3:
                found = (p, w, rec)
                break
        if found:
            break
    if found:
        p, w, rec = found
        c_real = w.certify()
    else:   # no seed pays slack: a record with a fractional slack written into it serves as well
        p = synthetic.generate("mini", 0, gap=1e-4)
        w = _solve(p); rec = copy.deepcopy(w.getRawResults())
        rec.slackvars_real[0, 0, 2, 0] = 0.375
        c_real = w.certify(rec)
    h = oracle.from_params(p)
    c_int = w.certify(rec, use_real_slack=False)
    vr, objr = _check(oracle, h, c_real, rec, real=True)
    vi, obji = _check(oracle, h, c_int, rec, real=False)
    assert abs((c_int.objective - c_real.objective) - (obji - objr)) <= 1e-9 * max(1.0, abs(objr))
    assert abs((c_int.max_violation - c_real.max_violation) - (vi - vr)) <= 1e-9
    assert c_int.raw != c_real.raw
    oracle.free(h)


def test_batch_equals_single_certificates():
    ps = [synthetic.generate("cfg3", 3000 + k, gap=1e-2) for k in range(256)]
    ws = []
    for p in ps:
        w = P.CplexWrapper(); w.resetParameters(p); ws.append(w)
    st = P.solve_batch(ws, inflight=128)
    certs = P.certify_batch(ws)
    nsol = 0
    for w, s, c in zip(ws, st, certs):
        if s == P.OptimizationStatus.SUCCESS:
            nsol += 1
            assert c.status == 0 and c.raw == w.certify().raw
            assert c.max_violation < 1e-5, c
        else:
            assert c.status == 1
    assert nsol >= 250
    # a second stream of the same shape after the certificates reuses the solver's device context
    st2 = P.solve_batch(ws, inflight=128)
    assert ws[0].lastTiming()["context_built"] is False
    assert [int(a) for a in st2] == [int(a) for a in st]
    # mixed shapes and handles without a solution in one call
    a = P.CplexWrapper(); a.resetParameters(synthetic.generate("mini", 0)); assert a.callCplex() == 0
    b = P.CplexWrapper(); b.resetParameters(synthetic.generate("mini3", 0)); assert b.callCplex() == 0
    e = P.CplexWrapper(); e.resetParameters(synthetic.generate("mini", 1)); assert e._push_inputs() == 0
    mixed = P.certify_batch([a, e, b, ws[0], e])
    assert [m.status for m in mixed] == [0, 1, 0, 0, 1]
    assert mixed[0].raw == a.certify().raw and mixed[2].raw == b.certify().raw and mixed[3].raw == ws[0].certify().raw
    assert mixed[0].rows == a.rawSizes()["rows"] and mixed[2].rows == b.rawSizes()["rows"]


def test_repeats_are_identical_and_a_time_limited_incumbent_certifies(oracle):
    p = synthetic.generate("cfg5", 11, gap=1e-9, max_time=0.5)
    w = P.CplexWrapper(); w.resetParameters(p)
    st = w.callCplex()
    if st != P.OptimizationStatus.SUCCESS:
        pytest.skip("no incumbent within the limit")
    assert w.getSolutionProperties().status in (101, 102, 107)
    c1 = w.certify(); c2 = w.certify()
    assert c1.raw == c2.raw
    h = oracle.from_params(p)
    _check(oracle, h, c1, w.getRawResults())
    oracle.free(h)
    assert c1.max_violation < 1e-5 and c1.rows == w.rawSizes()["rows"]


def test_a_long_horizon_is_read_from_global_memory(oracle):
    p = synthetic.generate((2, 140, 16, 1, 0), 0, gap=0.5, max_time=2.0)    # 12 x C x N doubles exceed the staged arrays
    w = P.CplexWrapper(); w.resetParameters(p)
    assert w._push_inputs() == 0
    rng = np.random.default_rng(5)
    r = P.RawResults(*_dims(p))
    for n in ("u_x", "u_y", "pos_x", "vel_x", "acc_x", "pos_y", "vel_y", "acc_y", "pos_x_front_UB", "pos_x_front_LB", "pos_y_front_UB", "pos_y_front_LB"):
        getattr(r, n)[...] = rng.normal(size=getattr(r, n).shape)
    for n in ("notWithinEnvironmentRear", "notWithinEnvironmentFrontUbUb", "notWithinEnvironmentFrontLbUb", "notWithinEnvironmentFrontUbLb",
              "notWithinEnvironmentFrontLbLb", "active_region", "region_change_not_allowed_x_positive", "region_change_not_allowed_y_positive",
              "region_change_not_allowed_x_negative", "region_change_not_allowed_y_negative", "region_change_not_allowed_combined",
              "car2car_collision"):
        a = getattr(r, n); a[...] = rng.integers(0, 2, size=a.shape)
    r.slackvars[...] = 0; r.slackvars_real[...] = rng.uniform(0, 1, size=r.slackvars_real.shape)
    r.deltacc[...] = 0; r.deltacc_front[...] = 0; r.slackvarsObstacle[...] = 0; r.slackvarsObstacle_front[...] = 0
    h = oracle.from_params(p)
    _check(oracle, h, w.certify(r), r)
    oracle.free(h)


def test_planner_with_a_certify_tolerance_plans_the_same():
    from planner_miqp_amd import planner_core as K
    S = dict(K.DefaultSettings(), warmstartType=P.WarmstartType.RECEDING_HORIZON_WARMSTART, nr_regions=32)
    lanes = ([[0, 0], [100, 0]], [[0, 3.5], [100, 3.5]])
    runs = []
    for tol in (None, 1e-5):
        pl = K.MiqpPlanner(S) if tol is None else K.MiqpPlanner(S, certify_tolerance=tol)
        cars = [pl.AddCar([0, 5.0, 0, 0, 0.0, 0], lanes[0], 8.0, 10.0), pl.AddCar([4.0, 6.0, 0, 3.5, 0.0, 0], lanes[1], 6.0, 10.0)]
        ts = pl.GetTs(); out = []
        for step in range(3):
            assert pl.Plan(step * ts), (step, pl.status, pl.lastError)
            if tol is not None:
                assert pl.certificate.status == 0 and pl.certificate.max_violation <= tol and pl.lastError == ""
            trajs = [pl.GetRawCMiqpTrajectory(c, step * ts) for c in cars]
            out.append(trajs)
            for c, t in zip(cars, trajs):
                pl.UpdateCar(c, [t[1, 1], t[1, 3], t[1, 5], t[1, 2], t[1, 4], t[1, 6]], lanes[c], (step + 1) * ts)
        runs.append(out)
    for a, b in zip(runs[0], runs[1]):
        for ta, tb in zip(a, b):
            assert np.array_equal(ta, tb)
    # a tolerance no solution meets turns the plan into a failure with a message
    pl = K.MiqpPlanner(S, certify_tolerance=-1.0)
    pl.AddCar([0, 5.0, 0, 0, 0.0, 0], lanes[0], 8.0, 10.0)
    assert not pl.Plan(0.0) and "certificate" in pl.lastError

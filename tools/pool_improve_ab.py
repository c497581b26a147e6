#!/usr/bin/env python3
"""The climb of a filtered solution pool (miqp_solver_pool_improve): what it gains, and what it costs against its host replay.

  python tools/pool_improve_ab.py [--cfg cfg4] [--seeds 16] [--gap 1e-4] [--capacity 16] [--filter 12] [--passes 8] [--cost-seed 9] [--runs 7]

Quality: per seed one solve with the filtered pool and one improveSolutionPool(passes) - the found objectives of the non-incumbent entries before
and after, the passes used and the neighbours solved.
Cost, on --cost-seed: the device-resident loop (A) against the host replay (B) - pool_moves per entry on the host, all neighbours of a pass through
ONE miqp_solver_solve_decisions call (one upload and one download of all records per pass), argmin and acceptance on the host; the same answers,
which the tool checks (objective bytes and decision bytes).  Every run of either side starts from the pool as found, which a fresh solve of the same
wrapper restores; that solve's own device time (lastTiming solve_s) is the yardstick printed beside.  One warm-up of each side, then --runs runs,
ALTERNATING A and B; median (min .. max) of the host wall clock around the call(s) and of the library's own figures (miqp_solver_last_timing
out[0] the whole call less what miqp_solver_last_setup reports for the device context, out[1] of which on the device; B: summed over its calls).
Both sides ask for the fixed-batch context, which the solve in front of every run may replace: the first call of either side then pays the
rebuild, which the host wall clock includes.  Needs an MI355X."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg", default="cfg4")
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--gap", type=float, default=1e-4)
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--filter", type=int, default=12)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--cost-seed", type=int, default=9)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import planner_miqp_amd as P
    from planner_miqp_amd import synthetic

    def solved(seed):
        w = P.CplexWrapper(); w.resetParameters(synthetic.generate(a.cfg, seed, gap=a.gap))
        assert w.setSolutionPool(a.capacity) == 0 and w.setSolutionPoolFilter(a.filter) == 0
        st = w.callCplex()
        assert st == P.OptimizationStatus.SUCCESS, (seed, st)
        return w

    def timing(w):
        t = (C.c_double * 6)()
        w._L.miqp_solver_last_timing(w._h, t)
        return list(t)

    def fmt(v):
        return " ".join("%.1f" % x for x in v)

    print("quality: %s seeds 0 .. %d, gap %g, capacity %d, filter %d, max_passes %d" % (a.cfg, a.seeds - 1, a.gap, a.capacity, a.filter, a.passes))
    for seed in range(a.seeds):
        w = solved(seed)
        found = w.solutionPoolFound()
        rc, before, after, moves, status = w.improveSolutionPool(a.passes)
        assert rc >= 0, rc
        t = timing(w)
        print("seed %2d: %2d entries, %2d moved, %d passes%s, %5d neighbours, device %7.3f ms | incumbent %.1f -> %.1f | others found: %s | after: %s"
              % (seed, len(found), rc, t[2], " (still moving)" if t[5] else "", t[3], 1e3 * t[1], found[0], after[0] if status[0] == 0 else found[0], fmt(found[1:]),
                 fmt([x if s == 0 else f for x, s, f in zip(after[1:], status[1:], found[1:])])))

    w = solved(a.cost_seed)
    d = (C.c_int * 6)()
    assert w._L.miqp_solver_get_dims(w._h, d) == 0
    Cn, N, O = d[0], d[1], d[4]
    w2 = P.CplexWrapper(); w2.resetParameters(synthetic.generate(a.cfg, a.cost_seed, gap=a.gap))   # the replay's handle: its calls leave the pool of w alone

    def restore():
        assert w.callCplex() == P.OptimizationStatus.SUCCESS
        return w.lastTiming()["solve_s"]

    def side_a():
        t0 = time.perf_counter()
        rc, before, after, moves, status = w.improveSolutionPool(a.passes)
        dt = time.perf_counter() - t0
        assert rc >= 0
        t = timing(w)
        t[0] -= w.lastTiming()["context_s"]
        dec = [w.solutionPoolFoundDecisions(k) for k in range(w.solutionPoolCount())]
        return dt, t[0], t[1], (after.tobytes(), b"".join(x.tobytes() for x in dec), t[2], t[3])

    def side_b():
        cur = [w.solutionPoolFoundDecisions(k) for k in range(w.solutionPoolCount())]
        lib = dev = 0.0
        t0 = time.perf_counter()
        rc, st, obj, viol, it, route, best = w2.solveDecisions(np.stack(cur))
        assert rc == 0
        t = timing(w2); lib += t[0] - w2.lastTiming()["context_s"]; dev += t[1]
        curobj, active, status = obj.copy(), [x == 0 for x in st], st.copy()
        passes = nb = 0
        for p in range(a.passes):
            lists = [P.pool_moves(Cn, N, O, a.filter, cur[k]) if active[k] else np.zeros((0, 4), dtype=np.int32) for k in range(len(cur))]
            total = sum(len(m) for m in lists)
            if total == 0:
                break
            recs = np.concatenate([np.repeat(cur[k][None, :], len(mv), axis=0) for k, mv in enumerate(lists) if len(mv)])
            q = 0
            for mv in lists:
                for first, stride, count, value in mv:
                    recs[q, first:first + count * stride:stride] = value
                    q += 1
            rc, st, obj, viol, it, route, best = w2.solveDecisions(recs)
            assert rc == 0
            t = timing(w2); lib += t[0] - w2.lastTiming()["context_s"]; dev += t[1]
            passes += 1; nb += total
            q, moved = 0, False
            for k, mv in enumerate(lists):
                o = np.where(st[q:q + len(mv)] == 0, obj[q:q + len(mv)], np.inf)
                bj = int(np.argmin(o)) if len(mv) else -1
                active[k] = bool(bj >= 0 and np.isfinite(o[bj]) and curobj[k] - o[bj] > 1e-9 * (1.0 + abs(curobj[k])))
                if active[k]:
                    first, stride, count, value = mv[bj]
                    cur[k][first:first + count * stride:stride] = value
                    curobj[k] = o[bj]; moved = True
                q += len(mv)
            if not moved:
                break
        dt = time.perf_counter() - t0
        return dt, lib, dev, (curobj.tobytes(), b"".join(x.tobytes() for x in cur), passes, nb)

    ra, rb, ys = [], [], []
    for run in range(a.runs + 1):
        ys.append(restore()); ra_ = side_a()
        ys.append(restore()); rb_ = side_b()
        assert ra_[3] == rb_[3], "the device-resident loop and its host replay disagree"
        if run > 0:   # (run 0: the warm-up of both sides)
            ra.append(ra_); rb.append(rb_)

    def ms(v):
        return "median %9.3f ms (min %9.3f .. max %9.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
    print("cost: %s seed %d, %d entries, %d passes, %d neighbours; %d alternating runs behind one warm-up; both sides leave the same objectives and decision bytes"
          % (a.cfg, a.cost_seed, w.solutionPoolCount(), ra[0][3][2], ra[0][3][3], a.runs))
    print("%-44s %s" % ("device time of the solve in front (yardstick)", ms(ys[2:])))
    for name, r in (("A  miqp_solver_pool_improve", ra), ("B  host replay over miqp_solver_solve_decisions", rb)):
        print("%-44s %s" % (name + ": host wall clock", ms([x[0] for x in r])))
        print("%-44s %s" % ("   library's out[0] less the context" + (", summed" if r is rb else ""), ms([x[1] for x in r])))
        print("%-44s %s" % ("   library's out[1] (device)" + (", summed" if r is rb else ""), ms([x[2] for x in r])))
    print("A against B: host wall clock %.2fx, library's out[0] less the context %.2fx, device %.2fx" % tuple(
        statistics.median([x[i] for x in rb]) / statistics.median([x[i] for x in ra]) for i in range(3)))


if __name__ == "__main__":
    main()

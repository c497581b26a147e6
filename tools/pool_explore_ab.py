#!/usr/bin/env python3
"""The step of a filtered solution pool across manoeuvre classes (miqp_solver_pool_explore): what it adds, and what it costs against its host replay.

  python tools/pool_explore_ab.py [--cfg cfg4] [--seeds 16] [--gap 1e-4] [--capacity 16] [--filter 12] [--passes 4] [--max-rel -1] [--climb 8]
                                  [--cost-seed 7] [--runs 7] [--distinct] [--settled] [--as-found]

Quality: per seed one solve with the filtered pool and one exploreSolutionPool(passes, max_rel) - the entries before and after, the passes and the
neighbours solved, the device time, the objectives of the added entries relative to the incumbent (objective / entry 0's found objective - 1) - and
the same ratios again behind improveSolutionPool(climb).
Cost, on --cost-seed: the device-resident loop (A) against the host replay (B) - pool_jumps per expanded entry on the host, all neighbours of a pass
through ONE miqp_solver_solve_decisions call (one upload and one download of all records per pass), the admission on the host with pool_signature;
the same answers, which the tool checks (objective bytes and decision bytes of the added entries).  Every run of either side starts from the pool as
found, which a fresh solve of the same wrapper restores; that solve's own device time (lastTiming solve_s) is the yardstick printed beside.  One
warm-up of each side, then --runs runs, ALTERNATING A and B; median (min .. max) of the host wall clock around the call(s) and of the library's own
figures (miqp_solver_last_timing out[0] the whole call less what miqp_solver_last_setup reports for the device context, out[1] of which on the
device; B: summed over its calls).
--distinct adds, per seed, the explore with distinct admission (miqp_solver_pool_explore_distinct) beside the plain one, each from the
pool as found: entries after the call, how many of them are real - left by solveSolutionPool - and how many that call merged away; and the device time
(miqp_solver_last_timing out[1]) of the two calls, median of --runs ALTERNATING runs behind one warm-up of each - in place of the cost comparison with
the host replay.  The passes run and the solves (miqp_solver_last_timing out[2], out[3]) of every call are printed beside.
--settled is --distinct with a third set of columns: the explore with settled admission (miqp_solver_pool_explore_settled).
--as-found prints, per seed, only what solveSolutionPool leaves of the pool AS FOUND, without any explore: "real" of a call less this number is what
the call added for good, and "merged away" less (found - this number) is what it added in vain.  Needs an MI355X."""
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
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--max-rel", type=float, default=-1.0)
    ap.add_argument("--climb", type=int, default=8)
    ap.add_argument("--cost-seed", type=int, default=7)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--distinct", action="store_true")
    ap.add_argument("--settled", action="store_true")
    ap.add_argument("--as-found", action="store_true")
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

    def dims(w):
        d = (C.c_int * 6)()
        assert w._L.miqp_solver_get_dims(w._h, d) == 0
        return d[0], d[1], d[4], d[5]

    def fmt(v):
        return " ".join("%+.3f" % x for x in v) if len(v) else "-"

    if a.as_found:
        print("the pool as found through solveSolutionPool, no explore: %s seeds 0 .. %d, gap %g, capacity %d, filter %d" % (a.cfg, a.seeds - 1, a.gap, a.capacity, a.filter))
        tot = [0, 0]
        for seed in range(a.seeds):
            w = solved(seed)
            n0 = w.solutionPoolCount()
            w.solveSolutionPool()
            tot[0] += n0; tot[1] += w.solutionPoolCount()
            print("seed %2d: %2d found -> %2d real, %2d merged" % (seed, n0, w.solutionPoolCount(), n0 - w.solutionPoolCount()))
        print("in all: %d found, %d real, %d merged" % (tot[0], tot[1], tot[0] - tot[1]))
        return

    print("quality: %s seeds 0 .. %d, gap %g, capacity %d, filter %d, max_passes %d, max_rel %g; behind it a climb of %d passes"
          % (a.cfg, a.seeds - 1, a.gap, a.capacity, a.filter, a.passes, a.max_rel, a.climb))
    for seed in range(a.seeds):
        w = solved(seed)
        n0 = w.solutionPoolCount()
        inc = w.solutionPoolFound()[0]
        rc, added = w.exploreSolutionPool(a.passes, a.max_rel)
        assert rc >= 0, rc
        t = timing(w) if n0 < a.capacity else [0.0] * 6   # (a full pool: no device work, the timing is still the solve's)
        rel = [x["objective"] / inc - 1.0 for x in added]
        crc, before, after, moves, status = w.improveSolutionPool(a.climb)
        assert crc >= 0, crc
        rel2 = [after[n0 + k] / after[0] - 1.0 for k in range(rc)]
        print("seed %2d: %2d -> %2d entries, %d passes%s, %5d neighbours, device %8.3f ms | incumbent %.1f | added, relative to it: %s | behind the climb (%d moved, incumbent %.1f): %s"
              % (seed, n0, n0 + rc, t[2], " (still adding)" if t[5] else "", t[3], 1e3 * t[1], inc, fmt(rel), crc, after[0], fmt(rel2)))

    if a.distinct or a.settled:
        modes = ["plain", "distinct"] + (["settled"] if a.settled else [])
        print("%s admission against the plain call, per seed and call: entries after the call, passes run, solves, real (left by solveSolutionPool), merged away; device ms, median of %d alternating runs"
              % (" and ".join(modes[1:]), a.runs))
        tot = {m: [0, 0] for m in modes}
        for seed in range(a.seeds):
            w = solved(seed)
            n0 = w.solutionPoolCount()
            row, dev = {}, {m: [] for m in modes}
            for run in range(a.runs + 1):
                for mode in modes:
                    if run or mode != modes[0]:   # (every call starts from the pool as found: a fresh solve of the same wrapper restores it)
                        assert w.callCplex() == P.OptimizationStatus.SUCCESS
                    rc, added = w.exploreSolutionPool(a.passes, a.max_rel, distinct=mode == "distinct", settled=mode == "settled")
                    assert rc >= 0, (seed, mode, rc)
                    t = timing(w) if n0 < a.capacity else [0.0] * 6   # (a full pool: no device work, the timing is still the solve's)
                    if run > 0 and n0 < a.capacity:   # (run 0: the warm-up of every call)
                        dev[mode].append(t[1])
                    if run == a.runs:
                        n1 = w.solutionPoolCount()
                        w.solveSolutionPool()
                        row[mode] = (n1, w.solutionPoolCount(), int(t[2]), int(t[3]))
            for mode in modes:
                tot[mode][0] += row[mode][0] - n0; tot[mode][1] += row[mode][0] - row[mode][1]
            med = {m: 1e3 * statistics.median(v) if v else 0.0 for m, v in dev.items()}
            print("seed %2d: %2d found | " % (seed, n0) + " | ".join(
                "%s -> %2d, %d passes, %5d solves -> %2d real, %2d merged, %8.3f ms" % (m, row[m][0], row[m][2], row[m][3], row[m][1], row[m][0] - row[m][1], med[m]) for m in modes)
                + " | " + ", ".join("%s / plain %s" % (m, "%.2fx" % (med[m] / med["plain"]) if med["plain"] > 0 else "-") for m in modes[1:]))
        print("in all: " + "; ".join("%s added %d, of which %d merged away" % (m, tot[m][0], tot[m][1]) for m in modes))
        return

    w = solved(a.cost_seed)
    Cn, N, O, L = dims(w)
    w2 = P.CplexWrapper(); w2.resetParameters(synthetic.generate(a.cfg, a.cost_seed, gap=a.gap))   # the replay's handle: its calls leave the pool of w alone

    def restore():
        assert w.callCplex() == P.OptimizationStatus.SUCCESS
        return w.lastTiming()["solve_s"]

    def side_a():
        n0 = w.solutionPoolCount()
        t0 = time.perf_counter()
        rc, added = w.exploreSolutionPool(a.passes, a.max_rel)
        dt = time.perf_counter() - t0
        assert rc >= 0
        t = timing(w)
        t[0] -= w.lastTiming()["context_s"]
        dec = [w.solutionPoolFoundDecisions(k) for k in range(n0, w.solutionPoolCount())]
        return dt, t[0], t[1], (np.array([x["objective"] for x in added]).tobytes(), b"".join(x.tobytes() for x in dec), t[2], t[3])

    def side_b():
        dec = [w.solutionPoolFoundDecisions(k) for k in range(w.solutionPoolCount())]
        obj0 = np.float64(w.solutionPoolFound()[0])
        n0 = len(dec)
        lib = dev = 0.0
        t0 = time.perf_counter()
        sigs = [P.pool_signature(Cn, N, O, a.filter, d).tobytes() for d in dec]
        objs, expand = [], list(range(n0))
        passes = nb = 0
        for p in range(a.passes):
            if len(dec) >= a.capacity:
                break
            lists = [P.pool_jumps(Cn, N, O, L, a.filter, dec[k]) for k in expand]
            total = sum(len(m) for m in lists)
            if total == 0:
                break
            recs = np.concatenate([np.repeat(dec[k][None, :], len(mv), axis=0) for k, mv in zip(expand, lists) if len(mv)])
            q = 0
            for mv in lists:
                for first, stride, count, value in mv:
                    recs[q, first:first + count * stride:stride] = value
                    q += 1
            rc, st, obj, viol, it, route, best = w2.solveDecisions(recs)
            assert rc == 0
            t = timing(w2); lib += t[0] - w2.lastTiming()["context_s"]; dev += t[1]
            passes += 1; nb += total
            new = []
            for g in np.lexsort((np.arange(total), obj)):
                if len(dec) >= a.capacity:
                    break
                if st[g] != 0 or (a.max_rel >= 0 and not obj[g] - obj0 <= np.float64(a.max_rel) * abs(obj0)):
                    continue
                sg = P.pool_signature(Cn, N, O, a.filter, recs[g]).tobytes()
                if sg in sigs:
                    continue
                new.append(len(dec)); dec.append(recs[g].copy()); sigs.append(sg); objs.append(obj[g])
            if not new:
                break
            expand = new
        dt = time.perf_counter() - t0
        return dt, lib, dev, (np.array(objs).tobytes(), b"".join(x.tobytes() for x in dec[n0:]), passes, nb)

    ra, rb, ys = [], [], []
    for run in range(a.runs + 1):
        ys.append(restore()); ra_ = side_a()
        ys.append(restore()); rb_ = side_b()
        assert ra_[3] == rb_[3], "the device-resident loop and its host replay disagree"
        if run > 0:   # (run 0: the warm-up of both sides)
            ra.append(ra_); rb.append(rb_)

    def ms(v):
        return "median %9.3f ms (min %9.3f .. max %9.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
    print("cost: %s seed %d, %d entries found, %d passes, %d neighbours; %d alternating runs behind one warm-up; both sides add the same objectives and decision bytes"
          % (a.cfg, a.cost_seed, w.solutionPoolCount(), ra[0][3][2], ra[0][3][3], a.runs))
    print("%-44s %s" % ("device time of the solve in front (yardstick)", ms(ys[2:])))
    for name, r in (("A  miqp_solver_pool_explore", ra), ("B  host replay over miqp_solver_solve_decisions", rb)):
        print("%-44s %s" % (name + ": host wall clock", ms([x[0] for x in r])))
        print("%-44s %s" % ("   library's out[0] less the context" + (", summed" if r is rb else ""), ms([x[1] for x in r])))
        print("%-44s %s" % ("   library's out[1] (device)" + (", summed" if r is rb else ""), ms([x[2] for x in r])))
    print("A against B: host wall clock %.2fx, library's out[0] less the context %.2fx, device %.2fx" % tuple(
        statistics.median([x[i] for x in rb]) / statistics.median([x[i] for x in ra]) for i in range(3)))


if __name__ == "__main__":
    main()

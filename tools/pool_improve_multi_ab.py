#!/usr/bin/env python3
"""The climb of the filtered pools of a drained queue: ONE miqp_solver_pool_improve_multi (A) against the loop of miqp_solver_pool_improve (B).

  python tools/pool_improve_multi_ab.py [--cfg cfg4] [--seeds 16] [--gap 1e-4] [--capacity 16] [--filter 12] [--passes 8] [--runs 7] [--only-b]

The --seeds instances are solved with the filtered pool on two twin sets of wrappers.  A: improve_solution_pools on set one; B: improveSolutionPool
per wrapper of set two.  Every run of either side starts from the pools as found, which a fresh solve of every wrapper of that set restores
(outside the timed part).  One warm-up of each side, then --runs runs, ALTERNATING A and B; median (min .. max) of
  host wall clock      around the call(s), seen from Python
  ... less the context the same less what miqp_solver_last_setup reports for the device context (the solves in front leave another context: the first
                       call of either side rebuilds it; B's later calls find it)
  library's out[1]     device time between the events of every pass (B: summed over the handles)
  passes               A: passes of the call (the most any handle took); B: summed over the handles (each handle's pass is a chain of launches
                       and a host synchronisation of its own)
and a check, every run, that both sides leave the same bytes: after / moves / status of every entry, every decision record, out[2 .. 5] per handle.
--only-b runs side B alone (the single-handle path, e.g. with the library of the parent commit: that path must not move).  Needs an MI355X."""
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
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--only-b", action="store_true")
    a = ap.parse_args()
    import planner_miqp_amd as P
    from planner_miqp_amd import synthetic

    def fresh():
        ws = []
        for seed in range(a.seeds):
            w = P.CplexWrapper(); w.resetParameters(synthetic.generate(a.cfg, seed, gap=a.gap))
            assert w.setSolutionPool(a.capacity) == 0 and w.setSolutionPoolFilter(a.filter) == 0
            ws.append(w)
        return ws

    def restore(ws):
        for seed, w in enumerate(ws):
            st = w.callCplex()
            assert st == P.OptimizationStatus.SUCCESS, (seed, st)

    def timing(w):
        t = (C.c_double * 6)()
        w._L.miqp_solver_last_timing(w._h, t)
        return list(t)

    def left(w, answer):
        moved, before, after, moves, status = answer
        dec = b"".join(w.solutionPoolFoundDecisions(k).tobytes() for k in range(w.solutionPoolCount()))
        return (moved, before.tobytes(), after.tobytes(), moves.tobytes(), status.tobytes(), dec, w.solutionPoolFound().tobytes(), tuple(timing(w)[2:6]))

    def side_a(ws):
        t0 = time.perf_counter()
        res = P.improve_solution_pools(ws, max_passes=a.passes)
        dt = time.perf_counter() - t0
        t = timing(ws[0])
        return dt, dt - ws[0].lastTiming()["context_s"], t[1], max(timing(w)[2] for w in ws), [left(w, r) for w, r in zip(ws, res)]

    def side_b(ws):
        ctx = dev = 0.0
        passes, out = 0, []
        t0 = time.perf_counter()
        for w in ws:
            r = w.improveSolutionPool(a.passes)
            assert r[0] >= 0, r[0]
            t = timing(w)
            ctx += w.lastTiming()["context_s"]; dev += t[1]; passes += t[2]
            out.append(r)
        dt = time.perf_counter() - t0
        return dt, dt - ctx, dev, passes, [left(w, r) for w, r in zip(ws, out)]

    one, two = (None if a.only_b else fresh()), fresh()
    ra, rb = [], []
    for run in range(a.runs + 1):
        if one is not None:
            restore(one); ra_ = side_a(one)
        restore(two); rb_ = side_b(two)
        if one is not None:
            assert ra_[4] == rb_[4], "one call over all handles and the loop of single calls disagree"
        if run > 0:   # (run 0: the warm-up of both sides)
            rb.append(rb_)
            if one is not None:
                ra.append(ra_)

    def ms(v):
        return "median %9.3f ms (min %9.3f .. max %9.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
    st = rb[0][4]
    print("%s seeds 0 .. %d, gap %g, capacity %d, filter %d, max_passes %d: %d entries, %d moved, %d neighbours, passes per handle %s; %d alternating runs behind one warm-up%s"
          % (a.cfg, a.seeds - 1, a.gap, a.capacity, a.filter, a.passes, sum(len(x[4]) // 4 for x in st), sum(x[0] for x in st), int(sum(x[7][1] for x in st)),
             [int(x[7][0]) for x in st], a.runs, "" if a.only_b else "; both sides leave the same bytes in every run"))
    for name, r in (("A  one miqp_solver_pool_improve_multi", ra), ("B  loop of miqp_solver_pool_improve", rb)):
        if not r:
            continue
        print("%-40s %s" % (name + ": host wall clock", ms([x[0] for x in r])))
        print("%-40s %s" % ("   ... less the context set-up", ms([x[1] for x in r])))
        print("%-40s %s" % ("   library's out[1] (device)" + (", summed" if r is rb else ""), ms([x[2] for x in r])))
        print("%-40s %d" % ("   passes" + (", summed over the handles" if r is rb else " of the call"), r[0][3]))
    if ra:
        print("A against B (B / A): host wall clock %.2fx, less the context set-up %.2fx, device %.2fx" % tuple(
            statistics.median([x[i] for x in rb]) / statistics.median([x[i] for x in ra]) for i in range(3)))


if __name__ == "__main__":
    main()

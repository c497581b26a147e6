#!/usr/bin/env python3
"""The explore of the filtered pools of a drained queue: ONE miqp_solver_pool_explore_multi (A) against the loop of the single calls (B), per admission.

  python tools/pool_explore_multi_ab.py [--cfg cfg4] [--seeds 16] [--gap 1e-4] [--capacity 16] [--filter 12] [--passes 4] [--max-rel -1] [--runs 7]
                                        [--modes plain,distinct,settled] [--only-b]

The --seeds instances are solved with the filtered pool on two twin sets of wrappers.  A: explore_solution_pools on set one; B: exploreSolutionPool
per wrapper of set two.  Every run of either side starts from the pools as found, which a fresh solve of every wrapper of that set restores (outside
the timed part).  One warm-up of each side, then --runs runs, ALTERNATING A and B; median (min .. max) of
  host wall clock      around the call(s), seen from Python
  ... less the context the same less what miqp_solver_last_setup reports for the device context (the solves in front leave another context: the first
                       call of either side rebuilds it; B's later calls find it)
  library's out[1]     device time between the events of every pass (B: summed over the handles)
  passes, slices       A: passes and slices of the call; B: passes summed over the handles (each handle's pass is a chain of launches and at least
                       one host synchronisation of its own)
and a check, every run, that both sides leave the same bytes: the added records, every decision record, the found objectives, out[2 .. 5] and the
last error per handle.
--only-b runs side B alone (the single-handle path, e.g. from a checkout of the parent commit: that path must not move).  Needs an MI355X."""
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
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--modes", default="plain,distinct,settled")
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

    def left(w, answer, took_part):
        rc, added = answer
        dec = b"".join(w.solutionPoolFoundDecisions(k).tobytes() for k in range(w.solutionPoolCount()))
        rec = tuple(tuple(sorted((k, v if k != "objective" else float(v).hex()) for k, v in d.items())) for d in added)
        return (rc, rec, dec, w.solutionPoolFound().tobytes(), tuple(timing(w)[2:6]) if took_part else None, w.lastError())

    def side_a(ws, kw):
        part = [0 < w.solutionPoolCount() < a.capacity for w in ws]
        t0 = time.perf_counter()
        res = P.explore_solution_pools(ws, max_passes=a.passes, max_rel=a.max_rel, **kw)
        dt = time.perf_counter() - t0
        first = ws[part.index(True)]
        passes, slices = P.pool_explore_multi_last()
        return dt, dt - first.lastTiming()["context_s"], timing(first)[1], (passes, slices), [left(w, r, p) for w, r, p in zip(ws, res, part)]

    def side_b(ws, kw):
        part = [0 < w.solutionPoolCount() < a.capacity for w in ws]
        ctx = dev = 0.0
        passes, out = 0, []
        t0 = time.perf_counter()
        for w, p in zip(ws, part):
            r = w.exploreSolutionPool(a.passes, a.max_rel, **kw)
            assert r[0] >= 0, r[0]
            if p:
                t = timing(w)
                ctx += w.lastTiming()["context_s"]; dev += t[1]; passes += t[2]
            out.append(r)
        dt = time.perf_counter() - t0
        return dt, dt - ctx, dev, (int(passes), None), [left(w, r, p) for w, r, p in zip(ws, out, part)]

    def ms(v):
        return "median %9.3f ms (min %9.3f .. max %9.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))

    one, two = (None if a.only_b else fresh()), fresh()
    for mode in a.modes.split(","):
        kw = dict(distinct=mode == "distinct", settled=mode == "settled")
        ra, rb = [], []
        for run in range(a.runs + 1):
            if one is not None:
                restore(one); ra_ = side_a(one, kw)
            restore(two); rb_ = side_b(two, kw)
            if one is not None:
                assert ra_[4] == rb_[4], "%s: one call over all handles and the loop of single calls disagree" % mode
            if run > 0:   # (run 0: the warm-up of both sides)
                rb.append(rb_)
                if one is not None:
                    ra.append(ra_)
        st = rb[0][4]
        print("%s, %s seeds 0 .. %d, gap %g, capacity %d, filter %d, max_passes %d, max_rel %g: %d entries added, %d solves, passes per handle %s; %d alternating runs behind one warm-up%s"
              % (mode, a.cfg, a.seeds - 1, a.gap, a.capacity, a.filter, a.passes, a.max_rel, sum(x[0] for x in st), int(sum(x[4][1] for x in st if x[4])),
                 [int(x[4][0]) if x[4] else "-" for x in st], a.runs, "" if a.only_b else "; both sides leave the same bytes in every run"))
        for name, r in (("A  one miqp_solver_pool_explore_multi", ra), ("B  loop of the single call", rb)):
            if not r:
                continue
            print("%-40s %s" % (name + ": host wall clock", ms([x[0] for x in r])))
            print("%-40s %s" % ("   ... less the context set-up", ms([x[1] for x in r])))
            print("%-40s %s" % ("   library's out[1] (device)" + (", summed" if r is rb else ""), ms([x[2] for x in r])))
            if r is rb:
                print("%-40s %d" % ("   passes, summed over the handles", r[0][3][0]))
            else:
                print("%-40s %d passes, %d slices" % ("   of the call", r[0][3][0], r[0][3][1]))
        if ra:
            print("%s, A against B (A / B): host wall clock %.2f, less the context set-up %.2f, device %.2f" % ((mode,) + tuple(
                statistics.median([x[i] for x in ra]) / statistics.median([x[i] for x in rb]) for i in range(3))))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A receding horizon with a solution pool: does the search profit from last cycle's pool?  Per cycle three orders of the same calls:
  (a) solve alone
  (b) solve, then carry from the previous cycle's pool               (the order without starts)
  (c) carry into the EMPTY pool, then solve with max_starts = 16     (setSolutionPoolStarts: the carried records are MIP starts of the solve)

  python tools/pool_starts_demo.py [--cfg cfg4] [--seeds 12,5] [--cycles 4] [--gap 1e-4] [--capacity 16] [--filter 12] [--shift 1] [--runs 7] [--out FILE]

Cycle 0 is synthetic.generate(cfg, seed) and seeds the chain with solve + settled explore, as tools/pool_carry_demo.py does; cycle t + 1 is
synthetic.advance of cycle t along its solution.  The chain - the pool the next cycle carries from - is (b)'s wrapper, so the three orders of a cycle
read the same source.  Per order: the node relaxations and the rounds of the solve (miqp_solver_last_timing), median (min .. max) over --runs runs
behind one warm-up, the three orders ALTERNATING and every run on fresh wrappers, of the solve's host wall clock as the caller sees it ("raw"),
of that wall clock less the device-context set-up (miqp_solver_last_setup) and of its device time; in how many of the runs the solve rebuilt the
device context; the entries solveSolutionPool leaves; and for (c) the number of starts T with their places in the pool behind the solve.
THE RAW WALL CLOCK IS DOMINATED BY CONTEXT REBUILDS HERE: a solve finds its context only when the call before it on the device had the same shape.
A pool call (carry, explore, refinement) has another shape than a solve, and a solve with starts (5 + max_starts root records per instance) another
than one without (5) - so in this alternation every solve of (c) rebuilds (a carry ran just before it), and so does every solve behind another
wrapper's pool call.  The column says what each run paid; a planner that keeps solves and pool calls on one device pays it in every order.
Needs an MI355X."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg", default="cfg4")
    ap.add_argument("--seeds", default="12,5")
    ap.add_argument("--cycles", type=int, default=4)
    ap.add_argument("--gap", type=float, default=1e-4)
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--filter", type=int, default=12)
    ap.add_argument("--shift", type=int, default=1)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import planner_miqp_amd as P
    from planner_miqp_amd import synthetic

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fresh(p, starts=0):
        w = P.CplexWrapper(); w.resetParameters(p)
        assert w.setSolutionPool(a.capacity) == 0 and w.setSolutionPoolFilter(a.filter) == 0 and w.setSolutionPoolStarts(starts) == 0
        return w

    def solve(w):
        """the solve of w: (nodes, rounds, wall less context set-up, device seconds, raw wall, 1 when the context was rebuilt)"""
        t0 = time.perf_counter()
        st = w.callCplex()
        dt = time.perf_counter() - t0
        assert st == P.OptimizationStatus.SUCCESS, st
        t = w.lastTiming()
        return t["nodes"], t["ipm_launches"], dt - t["context_s"], t["solve_s"], dt, int(t["context_built"])

    def order_a(p, src):
        w = fresh(p)
        return w, solve(w), []

    def order_b(p, src):
        w = fresh(p)
        s = solve(w)
        assert w.carrySolutionPool(src, a.shift)[0] >= 0
        return w, s, []

    def order_c(p, src):
        w = fresh(p, P.pool_max())
        assert w._loaded()
        assert w.carrySolutionPool(src, a.shift)[0] >= 0
        s = solve(w)
        return w, s, w.solutionPoolStartsLast()

    def ms(v):
        return "%8.3f (%8.3f .. %8.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))

    for seed in [int(x) for x in a.seeds.split(",")]:
        say("%s seed %d, gap %g, capacity %d, filter %d, shift %d, %d cycles; times in ms, median (min .. max) of %d alternating runs behind one warm-up"
            % (a.cfg, seed, a.gap, a.capacity, a.filter, a.shift, a.cycles, a.runs))
        p = synthetic.generate(a.cfg, seed, gap=a.gap)
        chain = None
        for t in range(a.cycles):
            if chain is None:
                w = fresh(p); s = solve(w)
                rec, obj = w.getRawResults(), w.getSolutionProperties().objective
                assert w.exploreSolutionPool(4, -1.0, settled=True)[0] >= 0
                say("cycle %2d: objective %10.4f  solve alone: %d nodes in %d rounds; the chain is seeded by a settled explore (%d entries)" % (t, obj, s[0], s[1], w.solutionPoolCount()))
                chain = w
            else:
                orders = (("(a) solve alone       ", order_a), ("(b) solve, then carry ", order_b), ("(c) carry, then solve ", order_c))
                runs = {n: [] for n, _ in orders}
                last = {}
                for run in range(a.runs + 1):
                    for n, f in orders:
                        w, s, places = f(p, chain)
                        if run > 0:
                            runs[n].append(s)
                        last[n] = (w, s, places)
                rec, obj = last[orders[0][0]][0].getRawResults(), last[orders[0][0]][0].getSolutionProperties().objective
                say("cycle %2d: objective (a) %10.4f, carried from %d entries" % (t, obj, chain.solutionPoolCount()))
                for n, _ in orders:
                    w, s, places = last[n]
                    found = w.solutionPoolCount()
                    left = len(w.solveSolutionPool()[1])
                    nodes, rounds = sorted({x[0] for x in runs[n]}), sorted({x[1] for x in runs[n]})
                    say("          %s objective %10.4f  nodes %s rounds %s  wall raw %s (context rebuilt in %d of %d runs) less context %s device %s  entries %d, after solveSolutionPool %d%s"
                        % (n, w.getSolutionProperties().objective, nodes, rounds, ms([x[4] for x in runs[n]]), sum(x[5] for x in runs[n]), len(runs[n]),
                           ms([x[2] for x in runs[n]]), ms([x[3] for x in runs[n]]), found, left,
                           "  T %d places %s" % (len(places), places) if n.startswith("(c)") else ""))
                chain = order_b(p, chain)[0]   # (a pool as found: the wrappers above were refined)
            p = synthetic.advance(p, rec, a.shift)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The carry of the pools of a drained queue into the next cycle: ONE miqp_solver_pool_carry_multi (A) against the loop of the single calls (B).

  python tools/pool_carry_multi_ab.py [--cfg cfg4] [--seeds 16] [--gap 1e-4] [--capacity 16] [--filter 12] [--shift 1] [--max-rel -1] [--runs 7] [--only-b]

Every one of the --seeds instances is solved with the filtered pool and explored (settled): the SOURCES, which both sides only read.  Its destination
is synthetic.advance of it along its solution by --shift steps, solved on a fresh wrapper - on two twin sets of wrappers.  A: carry_solution_pools
on set one; B: carrySolutionPool per wrapper of set two.  Every run of either side starts from the pools as found, which a fresh solve of every
destination of that set restores (outside the timed part).  A seed whose destination does not solve, or whose destination's pool as found is not the same after every one of
four solves of it in the set-up, is named and left out: the comparison of the sides needs equal pools to start from.  One warm-up of each side, then --runs runs, ALTERNATING A and B; median (min .. max) of
  host wall clock      around the call(s), seen from Python
  ... less the context the same less what miqp_solver_last_setup reports for the device context (the solves in front leave another context: the first
                       call of either side rebuilds it; B's later calls find it)
  library's out[1]     device time between the events of the call (B: summed over the pairs)
  rounds, groups       A: the settle rounds and launch groups of the call; B: the launch groups summed over the pairs (each a chain of launches and a
                       host synchronisation of its own)
and a check, every run, that both sides leave the same bytes: the count, every `out` record, every decision record, the found objectives,
out[2 .. 5] and the last error per pair.  Pairs that take no part (nothing to carry, a full destination) are named.
--only-b runs side B alone (the single call, e.g. from a checkout of the parent commit: that path must not move).  Needs an MI355X."""
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
    ap.add_argument("--shift", type=int, default=1)
    ap.add_argument("--max-rel", type=float, default=-1.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--only-b", action="store_true")
    a = ap.parse_args()
    import planner_miqp_amd as P
    from planner_miqp_amd import synthetic

    def pooled(p):
        w = P.CplexWrapper(); w.resetParameters(p)
        assert w.setSolutionPool(a.capacity) == 0 and w.setSolutionPoolFilter(a.filter) == 0
        return w

    # the sources: solved, explored (settled); the parameters of their destinations
    srcs, nexts = [], []
    for seed in range(a.seeds):
        p = synthetic.generate(a.cfg, seed, gap=a.gap)
        w = pooled(p)
        st = w.callCplex()
        assert st == P.OptimizationStatus.SUCCESS, (seed, st)
        nexts.append(synthetic.advance(p, w.getRawResults(), a.shift))
        srcs.append(w)
    for seed, w in enumerate(srcs):
        rc, _ = w.exploreSolutionPool(settled=True)
        assert rc >= 0, (seed, rc)

    def restore(ws):
        for seed, w in enumerate(ws):
            st = w.callCplex()
            assert st == P.OptimizationStatus.SUCCESS, (seed, st)

    def as_found(w):
        return (b"".join(w.solutionPoolFoundDecisions(k).tobytes() for k in range(w.solutionPoolCount())), w.solutionPoolFound().tobytes())

    def timing(w):
        t = (C.c_double * 6)()
        w._L.miqp_solver_last_timing(w._h, t)
        return list(t)

    def takes_part(ws):
        return [s.solutionPoolCount() > 0 and w.solutionPoolCount() < a.capacity for s, w in zip(srcs, ws)]

    def left(w, answer, took_part):
        rc, out = answer
        dec = b"".join(w.solutionPoolFoundDecisions(k).tobytes() for k in range(w.solutionPoolCount()))
        rec = tuple(tuple(sorted((k, v if k != "objective" else float(v).hex()) for k, v in d.items())) for d in out)
        return (rc, rec, dec, w.solutionPoolFound().tobytes(), tuple(timing(w)[2:6]) if took_part else None, w.lastError())

    def side_a(ws):
        part = takes_part(ws)
        t0 = time.perf_counter()
        res = P.carry_solution_pools(ws, srcs, a.shift, a.max_rel)
        dt = time.perf_counter() - t0
        first = ws[part.index(True)]
        return dt, dt - first.lastTiming()["context_s"], timing(first)[1], P.pool_carry_multi_last(), [left(w, r, p) for w, r, p in zip(ws, res, part)]

    def side_b(ws):
        part = takes_part(ws)
        ctx = dev = 0.0
        groups, out = 0, []
        t0 = time.perf_counter()
        for w, s, p in zip(ws, srcs, part):
            r = w.carrySolutionPool(s, a.shift, a.max_rel)
            assert r[0] >= 0, r[0]
            if p:
                t = timing(w)
                ctx += w.lastTiming()["context_s"]; dev += t[1]; groups += t[2]
            out.append(r)
        dt = time.perf_counter() - t0
        return dt, dt - ctx, dev, (None, int(groups)), [left(w, r, p) for w, r, p in zip(ws, out, part)]

    def ms(v):
        return "median %9.3f ms (min %9.3f .. max %9.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))

    two = [pooled(p) for p in nexts]
    solved = [w.callCplex() == P.OptimizationStatus.SUCCESS for w in two]   # (a destination that does not solve one step on has no cycle to carry into)
    if not all(solved):
        print("seeds without a solved destination, left out: %s" % [k for k, ok in enumerate(solved) if not ok])
        srcs[:], nexts[:], two = ([x for x, ok in zip(v, solved) if ok] for v in (srcs, nexts, two))
    # the comparison of the two sides needs destinations whose solve leaves the same pool on either twin: a search whose pool as found differs
    # between two solves of one instance (the optimum is the same, the other leaves it met are not) is named and left out
    one = [pooled(p) for p in nexts]
    pools = [{as_found(w)} for w in two]
    for ws in (one, two, one):
        restore(ws)
        for k, w in enumerate(ws):
            pools[k].add(as_found(w))
    if any(len(x) > 1 for x in pools):
        print("seeds whose destination's pool as found differs between solves of the same instance, left out: %s" % [k for k, x in enumerate(pools) if len(x) > 1])
        srcs[:], nexts[:], one, two = ([x for x, y in zip(v, pools) if len(y) == 1] for v in (srcs, nexts, one, two))
    if a.only_b:
        one = None
    ra, rb = [], []
    for run in range(a.runs + 1):
        if one is not None:
            restore(one); fa = [as_found(w) for w in one]; ra_ = side_a(one)
        restore(two); fb = [as_found(w) for w in two]; rb_ = side_b(two)
        unequal = [k for k, (x, y) in enumerate(zip(fa, fb)) if x != y] if one is not None else []
        if unequal:   # (the solves, not the carry: these pairs start from different pools in this run and are not compared in it)
            print("run %d: the pools as found differ between the twin sets on pairs %s; they are not compared in this run" % (run, unequal))
        if one is not None and any(x != y for k, (x, y) in enumerate(zip(ra_[4], rb_[4])) if k not in unequal):
            names = ("count", "out records", "decision records", "found objectives", "out[2 .. 5]", "last error")
            for k, (x, y) in enumerate(zip(ra_[4], rb_[4])):
                for what, u, v in zip(names, x, y):
                    if u != v and k not in unequal:
                        print("pair %d, %s: A %s | B %s" % (k, what, u if what != "decision records" else len(u), v if what != "decision records" else len(v)))
            raise SystemExit("one call over all pairs and the loop of single calls disagree")
        if run > 0:   # (run 0: the warm-up of both sides)
            rb.append(rb_)
            if one is not None:
                ra.append(ra_)
    st = rb[0][4]
    print("%s seeds 0 .. %d, gap %g, capacity %d, filter %d, shift %d, max_rel %g: source entries %s, destination entries before %s; %d entries admitted, %d solves, rounds per pair %s; "
          "pairs that take no part: %s; %d alternating runs behind one warm-up%s"
          % (a.cfg, a.seeds - 1, a.gap, a.capacity, a.filter, a.shift, a.max_rel, [s.solutionPoolCount() for s in srcs], [len(x[3]) // 8 - x[0] for x in st], sum(x[0] for x in st),
             int(sum(x[4][1] for x in st if x[4])), [int(x[4][0]) if x[4] else "-" for x in st], [k for k, x in enumerate(st) if not x[4]] or "none", a.runs,
             "" if a.only_b else "; both sides leave the same bytes in every run"))
    for name, r in (("A  one miqp_solver_pool_carry_multi", ra), ("B  loop of the single call", rb)):
        if not r:
            continue
        print("%-40s %s" % (name + ": host wall clock", ms([x[0] for x in r])))
        print("%-40s %s" % ("   ... less the context set-up", ms([x[1] for x in r])))
        print("%-40s %s" % ("   library's out[1] (device)" + (", summed" if r is rb else ""), ms([x[2] for x in r])))
        if r is rb:
            print("%-40s %d" % ("   launch groups, summed over the pairs", r[0][3][1]))
        else:
            print("%-40s %d rounds, %d launch groups" % ("   of the call", r[0][3][0], r[0][3][1]))
    if ra:
        print("A against B (A / B): host wall clock %.2f, less the context set-up %.2f, device %.2f" % tuple(
            statistics.median([x[i] for x in ra]) / statistics.median([x[i] for x in rb]) for i in range(3)))


if __name__ == "__main__":
    main()

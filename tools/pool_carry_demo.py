#!/usr/bin/env python3
"""A receding horizon with a solution pool: what the pool holds behind each cycle's solve alone (a), behind solve + settled explore (b) and behind
solve + carry from the previous cycle's pool (c), and what (b) and (c) cost.

  python tools/pool_carry_demo.py [--cfg cfg4] [--seed 12] [--cycles 8] [--gap 1e-4] [--capacity 16] [--filter 12] [--max-rel -1] [--runs 7]

Cycle 0 is synthetic.generate(cfg, seed); cycle t + 1 is synthetic.advance of cycle t along its solution, one step on.  Every cycle is solved on fresh
wrappers (the solve is the same for all three: nothing here feeds it).  (c) is a chain: its pool of cycle 0 is seeded by one settled explore, its pool
of cycle t >= 1 is the solve's and what carrySolutionPool admits from the chain's pool of cycle t - 1.  CLASSES are the entries solveSolutionPool
leaves (it merges entries of one settled signature), counted on a twin so that the chain's pool stays as found.
Per cycle: the classes of (a), (b), (c), the statuses the carry gave the source entries, and - one warm-up, then --runs runs, (b) and (c) ALTERNATING,
each run on a freshly solved wrapper - median (min .. max) of the host wall clock less the device-context set-up (miqp_solver_last_setup) and of the
library's device time out[1]; the shares of the carry's device time in pool_shift_kernel and pool_carry_admit_kernel, from the call's own events
(pool_carry_last); and the carry against its host replay (pool_shift, solveDecisions, settleDecisions, pool_signature and the admission in Python),
which has to give the same statuses.  Needs an MI355X."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg", default="cfg4")
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--cycles", type=int, default=8)
    ap.add_argument("--gap", type=float, default=1e-4)
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--filter", type=int, default=12)
    ap.add_argument("--max-rel", type=float, default=-1.0)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    import planner_miqp_amd as P
    from planner_miqp_amd import synthetic

    def solved(p):
        w = P.CplexWrapper(); w.resetParameters(p)
        assert w.setSolutionPool(a.capacity) == 0 and w.setSolutionPoolFilter(a.filter) == 0
        st = w.callCplex()
        assert st == P.OptimizationStatus.SUCCESS, st
        return w

    def timing(w):
        t = (C.c_double * 6)()
        w._L.miqp_solver_last_timing(w._h, t)
        return list(t)

    def classes(make):
        """the entries the refinement leaves of the pool `make` builds on a fresh wrapper"""
        w = make()
        return len(w.solveSolutionPool()[1]), w.solutionPoolCount()

    def timed(call, w):
        t0 = time.perf_counter()
        r = call(w)
        dt = time.perf_counter() - t0
        return dt - w.lastTiming()["context_s"], timing(w)[1], r

    def within(obj0, obj):
        return a.max_rel < 0 or np.float64(obj) - np.float64(obj0) <= np.float64(a.max_rel) * abs(np.float64(obj0))

    def replay(p, src, dst):
        """the carry as host code; the statuses per source entry"""
        d = (C.c_int * 6)(); dst._L.miqp_solver_get_dims(dst._h, d)
        Cn, N, O = d[0], d[1], d[4]
        w = P.CplexWrapper(); w.resetParameters(p)
        rm, em = w.poolCarryMaps(src)
        sig = lambda x: P.pool_signature(Cn, N, O, a.filter, x).tobytes()   # noqa: E731
        own = [dst.solutionPoolFoundDecisions(k) for k in range(dst.solutionPoolCount())]
        found = list(dst.solutionPoolFound())
        sh = [P.pool_shift(Cn, N, O, 1, src.solutionPoolFoundDecisions(k), rm, em) for k in range(min(src.solutionPoolCount(), 16))]
        ok = [k for k in range(len(sh)) if sh[k][0]]
        status = [2] * len(sh)
        if len(own) >= a.capacity or not ok:
            return status
        _, st1, obj1, _, _, _, _ = w.solveDecisions(np.stack([sh[k][1] for k in ok]))
        _, st, _, _, _, _, _, settled, _ = w.settleDecisions(np.stack(own + [sh[k][1] for k in ok]))
        sigs, ssigs, n = [sig(x) for x in own], [sig(settled[j]) for j in range(len(own)) if st[j] == 0], len(own)
        for k in ok:
            status[k] = 1
        for i, k in sorted(((i, k) for i, k in enumerate(ok) if st1[i] == 0), key=lambda t: (obj1[t[0]], t[1])):
            j = len(own) + i
            if n > 0 and not within(found[0], obj1[i]):
                status[k] = 5
            elif sig(sh[k][1]) in sigs:
                status[k] = 3
            elif st[j] != 0 or sig(settled[j]) in ssigs:
                status[k] = 4
            elif n >= a.capacity:
                status[k] = 6
            else:
                status[k] = 0; sigs.append(sig(sh[k][1])); ssigs.append(sig(settled[j])); found.append(float(obj1[i])); n += 1
        return status

    def ms(v):
        return "%8.3f (%8.3f .. %8.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))

    explore = lambda w: w.exploreSolutionPool(4, a.max_rel, settled=True)   # noqa: E731
    print("%s seed %d, gap %g, capacity %d, filter %d, max_rel %g, %d cycles; times in ms, median (min .. max) of %d alternating runs behind one warm-up"
          % (a.cfg, a.seed, a.gap, a.capacity, a.filter, a.max_rel, a.cycles, a.runs))
    p = synthetic.generate(a.cfg, a.seed, gap=a.gap)
    chain = None   # (c)'s wrapper of the cycle before: its pool is what the next cycle carries
    for t in range(a.cycles):
        first = solved(p)
        rec = first.getRawResults()
        na = classes(lambda: solved(p))

        def with_explore():
            w = solved(p); assert explore(w)[0] >= 0
            return w
        nb = classes(with_explore)
        if chain is None:
            chain_now = with_explore()
            print("cycle %2d: objective %10.4f  classes (entries): solve %d (%d), + settled explore %d (%d); the chain is seeded by the explore"
                  % (t, first.getSolutionProperties().objective, na[0], na[1], nb[0], nb[1]))
        else:
            src = chain
            carry = lambda w: w.carrySolutionPool(src, 1, a.max_rel)   # noqa: E731

            def with_carry():
                w = solved(p); assert carry(w)[0] >= 0
                return w
            nc = classes(with_carry)
            tb, tc, shares = [], [], []
            for run in range(a.runs + 1):
                rb = timed(explore, solved(p)); rc = timed(carry, solved(p))
                if run > 0:
                    tb.append(rb); tc.append(rc)
                    k = P.pool_carry_last()
                    shares.append((k[0] / rc[1], k[1] / rc[1]))
            chain_now = with_carry()
            statuses = [o["status"] for o in rc[2][1]]
            w0 = solved(p)
            t0 = time.perf_counter(); want = replay(p, src, w0); t_replay = time.perf_counter() - t0
            assert want == statuses, (want, statuses)
            print("cycle %2d: objective %10.4f  classes (entries): solve %d (%d), + settled explore %d (%d), + carry %d (%d); carried from %d entries: statuses %s"
                  % (t, first.getSolutionProperties().objective, na[0], na[1], nb[0], nb[1], nc[0], nc[1], src.solutionPoolCount(), statuses))
            print("          explore: wall %s device %s" % (ms([x[0] for x in tb]), ms([x[1] for x in tb])))
            print("          carry:   wall %s device %s" % (ms([x[0] for x in tc]), ms([x[1] for x in tc])))
            print("          carry / explore: wall %.3f, device %.3f; of the carry's device time pool_shift_kernel %.4f, pool_carry_admit_kernel %.4f; host replay %.1f ms, the same statuses"
                  % (statistics.median([x[0] for x in tc]) / statistics.median([x[0] for x in tb]), statistics.median([x[1] for x in tc]) / statistics.median([x[1] for x in tb]),
                     statistics.median([s[0] for s in shares]), statistics.median([s[1] for s in shares]), 1e3 * t_replay))
        chain = chain_now
        p = synthetic.advance(p, rec, 1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The solution pool of one synthetic instance, entry by entry.

  python tools/solution_pool_demo.py --config cfg4 --seed 0 [--capacity 8] [--filter 12] [--gap 1e-4] [--runs 5]

Solves the instance with setSolutionPool(capacity), refines the kept entries with solveSolutionPool and prints per entry the objective as the search
found it, the refined one, the Hamming distance of its binaries to entry 0 (how different the manoeuvre is) and the worst violation the device
certificate finds for its record.  With --filter F the pool keeps one entry per signature under the families F (setSolutionPoolFilter; 12 = obstacle
sides and car/car order); per entry a short hash of its signature - under F, or under 12 with the filter off - shows which entries are one class.  With --runs it also times the solve with the pool off and on (device time of the solve from its own events, median
of the runs after one warm-up of each) and the refinement call.  Needs an MI355X."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="cfg4", help="a name of planner_miqp_amd.synthetic.CONFIGS")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--filter", type=int, default=0, help="families of the manoeuvre filter, a bit set 0 .. 31 (0: off)")
    ap.add_argument("--gap", type=float, default=1e-4)
    ap.add_argument("--runs", type=int, default=0, help="time the solve with the pool off and on, this many runs each")
    a = ap.parse_args()
    import hashlib
    import helpers as H
    import planner_miqp_amd as P
    from planner_miqp_amd import synthetic
    p = synthetic.generate(a.config, a.seed, gap=a.gap)
    w = P.CplexWrapper(); w.resetParameters(p)
    if w.setSolutionPool(a.capacity) != 0:
        sys.exit("capacity %d refused (0 .. %d)" % (a.capacity, P.pool_max()))
    if w.setSolutionPoolFilter(a.filter) != 0:
        sys.exit("filter %d refused (0 .. 31)" % a.filter)
    st = w.callCplex()
    props = w.getSolutionProperties()
    print("%s seed %d: status %s objective %.10f bound %.10f nodes %d, pool %d of %d, filter %d" % (a.config, a.seed, st.name, props.objective, props.best_bound, props.nodes, w.solutionPoolCount(), a.capacity, a.filter))
    if st != P.OptimizationStatus.SUCCESS:
        return
    fam = a.filter if a.filter else P.POOL_BY_OBSTACLE | P.POOL_BY_CAR_CAR
    kept, kept_found = w.solutionPoolCount(), w.solutionPoolFound()
    dec = [w.solutionPoolFoundDecisions(k) for k in range(kept)]
    cn, pairs = p.NumCars * p.NumSteps, p.NumCars * (p.NumCars - 1) // 2
    nobs = (len(dec[0]) - 6 * cn - 4 * pairs * p.NumSteps) // (5 * cn) if kept else 0   # (the obstacles the instance holds, from the length of its decision part)
    cls = [hashlib.sha1(P.pool_signature(p.NumCars, p.NumSteps, nobs, fam, d).tobytes()).hexdigest()[:8] for d in dec]
    print("as found: %d entries in %d classes under families %d" % (kept, len(set(cls)), fam))
    print("entry  found objective   signature")
    for k in range(kept):
        print("%5d  %16.10f  %s" % (k, kept_found[k], cls[k]))
    t = time.perf_counter()
    status, obj, viol, it, route = w.solveSolutionPool()
    t_ref = time.perf_counter() - t
    found = w.solutionPoolFound()   # behind the refinement, which merges entries that are one solution
    lt = w.lastTiming()
    recs = [w.solutionPoolRecord(k)[1] for k in range(len(found))]
    fields = H.BIN_FIELDS + ["car2car_collision"]
    print("refinement: %.3f ms host wall clock, %.3f ms on the device, %d launch groups" % (1e3 * t_ref, 1e3 * lt["ipm_s"], lt["ipm_launches"]))
    print("entry  found objective   refined objective  status  hamming to 0  certificate violation")
    for k, r in enumerate(recs):
        if r is None:
            print("%5d  %16.10f  %17s  %6d" % (k, found[k], "-", status[k]))
            continue
        ham = sum(int(np.sum(getattr(r, n) != getattr(recs[0], n))) for n in fields) if recs[0] is not None else -1
        cert = w.certify(r)
        print("%5d  %16.10f  %17.10f  %6d  %12d  %.3e" % (k, found[k], obj[k], status[k], ham, cert.max_violation))
    if a.runs > 0:
        def solve(cap):
            v = P.CplexWrapper(); v.resetParameters(p); v.setSolutionPool(cap); v.setSolutionPoolFilter(a.filter)
            t0 = time.perf_counter(); v.callCplex(); dt = time.perf_counter() - t0
            q = v.lastTiming()
            return dt, q["solve_s"], q["ipm_launches"]
        for cap in (0, a.capacity):
            solve(cap)
            runs = [solve(cap) for _ in range(a.runs)]
            print("solve with capacity %d filter %d: host median %.3f ms, device median %.3f ms (min %.3f, max %.3f), %d rounds" %
                  (cap, a.filter if cap else 0, 1e3 * statistics.median(r[0] for r in runs), 1e3 * statistics.median(r[1] for r in runs), 1e3 * min(r[1] for r in runs), 1e3 * max(r[1] for r in runs), runs[0][2]))


if __name__ == "__main__":
    main()

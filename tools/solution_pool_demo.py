#!/usr/bin/env python3
"""The solution pool of one synthetic instance, entry by entry.

  python tools/solution_pool_demo.py --config cfg4 --seed 0 [--capacity 8] [--gap 1e-4] [--runs 5]

Solves the instance with setSolutionPool(capacity), refines the kept entries with solveSolutionPool and prints per entry the objective as the search
found it, the refined one, the Hamming distance of its binaries to entry 0 (how different the manoeuvre is) and the worst violation the device
certificate finds for its record.  With --runs it also times the solve with the pool off and on (device time of the solve from its own events, median
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
    ap.add_argument("--gap", type=float, default=1e-4)
    ap.add_argument("--runs", type=int, default=0, help="time the solve with the pool off and on, this many runs each")
    a = ap.parse_args()
    import helpers as H
    import planner_miqp_amd as P
    from planner_miqp_amd import synthetic
    p = synthetic.generate(a.config, a.seed, gap=a.gap)
    w = P.CplexWrapper(); w.resetParameters(p)
    if w.setSolutionPool(a.capacity) != 0:
        sys.exit("capacity %d refused (0 .. %d)" % (a.capacity, P.pool_max()))
    st = w.callCplex()
    props = w.getSolutionProperties()
    print("%s seed %d: status %s objective %.10f bound %.10f nodes %d, pool %d of %d" % (a.config, a.seed, st.name, props.objective, props.best_bound, props.nodes, w.solutionPoolCount(), a.capacity))
    if st != P.OptimizationStatus.SUCCESS:
        return
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
            v = P.CplexWrapper(); v.resetParameters(p); v.setSolutionPool(cap)
            t0 = time.perf_counter(); v.callCplex(); dt = time.perf_counter() - t0
            q = v.lastTiming()
            return dt, q["solve_s"], q["ipm_launches"]
        for cap in (0, a.capacity):
            solve(cap)
            runs = [solve(cap) for _ in range(a.runs)]
            print("solve with capacity %d: host median %.3f ms, device median %.3f ms (min %.3f, max %.3f), %d rounds" %
                  (cap, 1e3 * statistics.median(r[0] for r in runs), 1e3 * statistics.median(r[1] for r in runs), 1e3 * min(r[1] for r in runs), 1e3 * max(r[1] for r in runs), runs[0][2]))


if __name__ == "__main__":
    main()

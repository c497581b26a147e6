#!/usr/bin/env python3
"""Refining the solution pools of a drained queue: a loop of miqp_solver_pool_solve over the handles against one miqp_solver_pool_solve_multi.

  python tools/pool_refine_ab.py [--n 256] [--cfg cfg3] [--gap 0.01] [--capacity 8] [--inflight 64] [--runs 5]

Two twin sets of handles on the same seeds are drained as a stream (solve_batch(inflight=...)) with a pool of `capacity` on every handle; set A is
then refined by the loop, set B by the one call.  Host wall clock around the C calls (ctypes, no numpy marshalling on either side), one warm-up of
each side, then `runs` runs each: median (min .. max).  Each side is timed as a block, never interleaved: the two ask for the device context in
different ways, and the context the stream left is rebuilt by the warm-up.  The warm-up is also the call that merges entries that are one solution,
so every timed run of either side refines the merged pools - the same entries on both sides, which the tool checks (counts and objective bytes).
Also printed: the library's own figures (miqp_solver_last_timing out[0] / out[1]: the loop's summed over its calls), how many of the loop's
calls rebuilt the device context (miqp_solver_last_setup out[2]), and the distinct own Layouts (P, EL) among the handles, which is what makes
them.  Needs an MI355X."""
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
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--cfg", default="cfg3")
    ap.add_argument("--gap", type=float, default=0.01)
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--inflight", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import planner_miqp_amd as P
    from planner_miqp_amd import synthetic
    from planner_miqp_amd.ctypes_types import FixedResultC
    L = P.load_library()
    ps = [synthetic.generate(a.cfg, seed, gap=a.gap) for seed in range(a.n)]
    sets = []
    for _ in range(2):
        ws = []
        for p in ps:
            w = P.CplexWrapper(); w.resetParameters(p)
            assert w.setSolutionPool(a.capacity) == 0
            ws.append(w)
        t = time.perf_counter()
        sts = P.solve_batch(ws, inflight=a.inflight)
        dt = time.perf_counter() - t
        assert all(st == P.OptimizationStatus.SUCCESS for st in sts), [int(s) for s in sts]
        print("stream of %d %s instances (gap %g, %d in flight, pool %d): %.3f s, %d pool entries kept" % (a.n, a.cfg, a.gap, a.inflight, a.capacity, dt, sum(w.solutionPoolCount() for w in ws)))
        sets.append(ws)
    A, B = sets
    cap = a.capacity
    out = (FixedResultC * (a.n * cap))()
    counts = (C.c_int * a.n)()
    hs = (C.c_void_p * a.n)(*[w._h for w in B])
    hA = [w._h for w in A]
    one = [C.cast(C.byref(out, h * cap * C.sizeof(FixedResultC)), C.POINTER(FixedResultC)) for h in range(a.n)]

    def loop():
        lib_s = dev_s = 0.0; rebuilt = 0
        t3 = (C.c_double * 6)(); u3 = (C.c_double * 3)()
        t = time.perf_counter()
        for h in range(a.n):
            m = L.miqp_solver_pool_solve(hA[h], one[h], cap)
            assert m >= 0, (h, m)
            counts[h] = m
            L.miqp_solver_last_timing(hA[h], t3); L.miqp_solver_last_setup(hA[h], u3)
            lib_s += t3[0]; dev_s += t3[1]; rebuilt += int(u3[2])
        return time.perf_counter() - t, lib_s, dev_s, rebuilt

    def multi():
        t = time.perf_counter()
        m = L.miqp_solver_pool_solve_multi(hs, a.n, out, cap, counts)
        dt = time.perf_counter() - t
        assert m >= 0, m
        tm = B[0].lastTiming()
        return dt, tm["solve_s"], tm["ipm_s"], int(tm["context_built"])

    def snapshot():
        return [(counts[h], bytes(np.array([out[h * cap + k].objective for k in range(counts[h])], dtype=np.float64).tobytes())) for h in range(a.n)]

    w0 = loop()
    ra = [loop() for _ in range(a.runs)]
    sa = snapshot()
    w1 = multi()
    rb = [multi() for _ in range(a.runs)]
    sb = snapshot()
    assert sa == sb, "the two sides disagree on the refined pools"
    entries = sum(c for c, _ in sb)

    def ms(v):
        return "median %9.3f ms (min %9.3f .. max %9.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
    lays = {}
    for p in ps:
        key = (int(np.asarray(p.possible_region).sum(1).max()), max(len(np.asarray(e).reshape(-1, 2)) for e in p.MultiEnvironmentConvexPolygon))
        lays[key] = lays.get(key, 0) + 1
    print("%d handles, %d entries left in all (the same on both sides, objectives equal as bytes); own Layouts (P, EL): %s" % (a.n, entries, sorted(lays.items())))
    print("warm-up: loop %.3f ms (%d context builds), one call %.3f ms (%d context builds)" % (1e3 * w0[0], w0[3], 1e3 * w1[0], w1[3]))
    print("%-36s %s" % ("", "host wall clock around the C calls, %d runs" % a.runs))
    print("%-36s %s  -> %.3f ms per handle" % ("loop of miqp_solver_pool_solve", ms([r[0] for r in ra]), 1e3 * statistics.median([r[0] for r in ra]) / a.n))
    print("%-36s %s" % ("  library's out[0], summed", ms([r[1] for r in ra])))
    print("%-36s %s" % ("  library's out[1] (device), summed", ms([r[2] for r in ra])))
    print("%-36s %s" % ("  context builds per run", sorted(r[3] for r in ra)))
    print("%-36s %s  -> %.3f ms per handle" % ("one miqp_solver_pool_solve_multi", ms([r[0] for r in rb]), 1e3 * statistics.median([r[0] for r in rb]) / a.n))
    print("%-36s %s" % ("  library's out[0]", ms([r[1] for r in rb])))
    print("%-36s %s" % ("  library's out[1] (device)", ms([r[2] for r in rb])))
    print("%-36s %s" % ("  context builds per run", sorted(r[3] for r in rb)))
    print("the one call against the loop: %.1fx" % (statistics.median([r[0] for r in ra]) / statistics.median([r[0] for r in rb])))


if __name__ == "__main__":
    main()

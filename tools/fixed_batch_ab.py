#!/usr/bin/env python3
"""n single solveFixed calls against one solveFixedBatch of the same records, on one instance.

  python tools/fixed_batch_ab.py --shape c2n20a --n 256 [--runs 7]

The records are the relax levels of the shape (tests/helpers.py: the regions of a feasible record asserted, parts of its leaf disjunctions
undecided), cycled to n entries.  Host wall clock around the calls, after one warm-up of each side (the device context is built there: the
two sides use contexts of different sizes, so each side is timed as a block, never interleaved).  Prints median and spread of both
sides, and of the batch call the part spent on the device (first launch group to last kernel, from device events) against the host.
Needs an MI355X and the CPU oracle (it provides the feasible record)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="c2n20a", help="a name of tests/helpers.py NODE_SHAPES")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    import helpers as H
    import oracle_lib
    import planner_miqp_amd as P
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    O = oracle_lib.Oracle(os.path.join(ROOT, "oracle", "_build", "liboracle.so"))
    p, h, dims, rec = H.node_instance(O, a.shape)
    levels = [r for r, _ in H.relax_levels(rec, H.RELAX_SEED[a.shape]).values()]
    records = [levels[k % len(levels)] for k in range(a.n)]
    w = P.CplexWrapper(); w.resetParameters(p)

    def loop():
        t = time.perf_counter()
        for r in records:
            w.solveFixed(r)
        return time.perf_counter() - t

    def batch():
        t = time.perf_counter()
        w.solveFixedBatch(records)
        dt = time.perf_counter() - t
        return dt, w.lastTiming()

    loop()
    t_loop = [loop() for _ in range(a.runs)]
    batch()
    runs = [batch() for _ in range(a.runs)]
    t_batch = [r[0] for r in runs]
    lib = [r[1]["solve_s"] for r in runs]; dev = [r[1]["ipm_s"] for r in runs]

    def ms(v):
        return "median %.3f ms (min %.3f, max %.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
    print("shape %s dims %s, n = %d (%d levels cycled), %d runs after one warm-up, chunk %d" % (a.shape, dims, a.n, len(levels), a.runs, P.fixed_batch_chunk()))
    print("loop of n solveFixed calls:  %s  -> %.3f ms per record" % (ms(t_loop), 1e3 * statistics.median(t_loop) / a.n))
    print("one solveFixedBatch call:    %s  -> %.3f ms per record" % (ms(t_batch), 1e3 * statistics.median(t_batch) / a.n))
    print("  of which inside the library %s, on the device %s: %.0f %% of the call in the launches, the rest host (marshalling, fix records, tables, download)"
          % (ms(lib), ms(dev), 100.0 * statistics.median(dev) / statistics.median(t_batch)))
    print("speed-up of the batch call over the loop: %.1fx" % (statistics.median(t_loop) / statistics.median(t_batch)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Every entry point that sends fix records through the fixed chain, in one fixed order, as one sha256 line per step.

  MIQP_GPU_LIB=<library> python tools/fixed_calls_dump.py OUT

Two builds of the library compute the same thing exactly when their files are identical.  Per seed 0 .. 3 of cfg4 (gap 1e-4, pool capacity 8,
filter 12), on fresh wrappers: the solve; solveDecisions, canonicalDecisions and settleDecisions of the found decisions; solveSolutionPool and
every pool record; solveFixedBatch of those records repeated to fixed_batch_chunk() + 3 entries; the climb at 8 passes; the explore at 4 passes;
the refinement again; the distinct and the settled explore at 4 passes, each on a fresh solve.  Then the three calls over many handles -
refinement, climb, fix records - on twin wrappers of all seeds.  A line covers the returned arrays, best, `added`, decision bytes, record bytes
or pool bytes, and last_timing[2 .. 5] of the step.  Needs an MI355X and no oracle."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEEDS, CAPACITY, FILTER = range(4), 8, 12


def main():
    out_path = sys.argv[1]
    import numpy as np
    import planner_miqp_amd as P
    from planner_miqp_amd import synthetic
    from planner_miqp_amd.ctypes_types import _RES_D, _RES_I
    lines = []

    def solved(seed):
        w = P.CplexWrapper(); w.resetParameters(synthetic.generate("cfg4", seed, gap=1e-4))
        assert w.setSolutionPool(CAPACITY) == 0 and w.setSolutionPoolFilter(FILTER) == 0
        assert w.callCplex() == P.OptimizationStatus.SUCCESS, seed
        return w

    def timing(w):
        t = (C.c_double * 6)()
        w._L.miqp_solver_last_timing(w._h, t)
        return np.array(list(t)[2:6]).tobytes()

    def rec_bytes(r):
        return b"" if r is None else b"".join(np.ascontiguousarray(getattr(r, n)).tobytes() for n in list(_RES_D) + list(_RES_I) + ["slackvars_real"])

    def pool_bytes(w):
        return b"".join(w.solutionPoolFoundDecisions(k).tobytes() for k in range(w.solutionPoolCount())) + w.solutionPoolFound().tobytes()

    def emit(tag, *parts):
        h = hashlib.sha256()
        for p in parts:
            h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
        lines.append("%-28s %s" % (tag, h.hexdigest()))

    def refine(w):
        res = w.solveSolutionPool()
        recs = [w.solutionPoolRecord(k) for k in range(len(res[0]))]
        return res, recs

    def refine_parts(w, res, recs):
        return list(res) + [np.array([rc for rc, _ in recs])] + [rec_bytes(r) for _, r in recs] + [pool_bytes(w), timing(w)]

    def fixed_parts(w, res):
        st = res[0]
        recs = [w.fixedBatchRecord(k) for k in range(len(st))]
        return list(res[:5]) + [np.array([res[5]]), np.array([rc for rc, _ in recs])] + [rec_bytes(r) for _, r in recs] + [timing(w)]

    lists = []
    for seed in SEEDS:
        w = solved(seed)
        emit("seed%d solve" % seed, np.array([w.getSolutionProperties().objective]), rec_bytes(w.getRawResults()), pool_bytes(w))
        dec = np.stack([w.solutionPoolFoundDecisions(k) for k in range(w.solutionPoolCount())])
        res = w.solveDecisions(dec)
        assert res[0] == 0
        emit("seed%d solve_decisions" % seed, *fixed_parts(w, res[1:]))
        res = w.canonicalDecisions(dec)
        assert res[0] == 0
        emit("seed%d canonical_decisions" % seed, *res[1:6], np.array([res[6]]), res[7], pool_bytes(w), timing(w))
        res = w.settleDecisions(dec)
        assert res[0] == 0
        emit("seed%d settle_decisions" % seed, *res[1:6], np.array([res[6]]), res[7], res[8], pool_bytes(w), timing(w))
        res, recs = refine(w)
        emit("seed%d pool_solve" % seed, *refine_parts(w, res, recs))
        records = [r for rc, r in recs if rc == 0]
        n = P.fixed_batch_chunk() + 3
        batch = [records[k % len(records)] for k in range(n)]
        emit("seed%d solve_fixed_batch" % seed, *fixed_parts(w, w.solveFixedBatch(batch)))
        lists.append(records)
        res = w.improveSolutionPool(8)
        assert res[0] >= 0
        emit("seed%d pool_improve" % seed, np.array([res[0]]), *res[1:], pool_bytes(w), timing(w))
        rc, added = w.exploreSolutionPool(4)
        assert rc >= 0
        emit("seed%d pool_explore" % seed, np.array([rc]), repr([sorted(a.items()) for a in added]).encode(), pool_bytes(w), timing(w))
        res, recs = refine(w)
        emit("seed%d pool_solve again" % seed, *refine_parts(w, res, recs))
        for mode in ("distinct", "settled"):
            w = solved(seed)
            rc, added = w.exploreSolutionPool(4, **{mode: True})
            assert rc >= 0
            emit("seed%d pool_explore %s" % (seed, mode), np.array([rc]), repr([sorted(a.items()) for a in added]).encode(), pool_bytes(w), timing(w))

    ws = [solved(seed) for seed in SEEDS]
    for h, res in enumerate(P.solve_solution_pools(ws)):
        emit("multi pool_solve h%d" % h, *refine_parts(ws[h], res, [ws[h].solutionPoolRecord(k) for k in range(len(res[0]))]))
    ws = [solved(seed) for seed in SEEDS]
    for h, res in enumerate(P.improve_solution_pools(ws, 8)):
        emit("multi pool_improve h%d" % h, np.array([res[0]]), *res[1:], pool_bytes(ws[h]), timing(ws[h]))
    ws = [solved(seed) for seed in SEEDS]
    many = [[l[k % len(l)] for k in range(300 + 7 * h)] for h, l in enumerate(lists)]   # (1242 nodes: handle 3 on both sides of a launch group)
    for h, res in enumerate(P.solve_fixed_multi(ws, many)):
        emit("multi solve_fixed h%d" % h, *fixed_parts(ws[h], res))

    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

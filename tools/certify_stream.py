"""A queue of synthetic instances streamed through the solver, then certified in one batch call against the raw big-M model.

  python tools/certify_stream.py --config cfg3 --n 2560 --inflight 1280 [--seed0 0] [--gap 0.01] [--limit 10]

Prints the number of certificates, the worst raw-row violation with its family and instance, and the seconds of the
certify call (host packing / upload / kernel, the last two from device events; they overlap) next to those of the stream."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402

import planner_miqp_amd as P  # noqa: E402
from planner_miqp_amd import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--n", type=int, default=2560)
    ap.add_argument("--inflight", type=int, default=1280)
    ap.add_argument("--seed0", type=int, default=0)
    ap.add_argument("--gap", type=float, default=0.01)
    ap.add_argument("--limit", type=float, default=10.0)
    ap.add_argument("--repeat", type=int, default=2, help="certify calls (the first allocates the staging buffers)")
    a = ap.parse_args()
    ws = []
    for k in range(a.n):
        w = P.CplexWrapper()
        w.resetParameters(synthetic.generate(a.config, a.seed0 + k, gap=a.gap, max_time=a.limit))
        ws.append(w)
    P.prepare_batch(ws)
    t = time.time()
    st = P.solve_batch(ws, inflight=a.inflight, prepared=True)
    made = P.materialize_results(ws)
    t_stream = time.time() - t
    solved = sum(1 for s in st if s == P.OptimizationStatus.SUCCESS)
    print("stream: %d instances of %s, %d in flight: %d solved, %.3f s (records of %d built inside)" % (a.n, a.config, a.inflight, solved, t_stream, made))
    for rep in range(max(1, a.repeat)):
        t = time.time()
        certs = P.certify_batch(ws)
        t_cert = time.time() - t
        tm = P.certify_last_timing()
        print("certify call %d: %.4f s wall = %.1f %% of the stream (packing %.6f s, upload %.6f s, kernel %.6f s; %.3f us kernel per record)"
              % (rep, t_cert, 100.0 * t_cert / max(t_stream, 1e-9), tm["pack_s"], tm["upload_s"], tm["kernel_s"], 1e6 * tm["kernel_s"] / max(1, solved)))
    ok = [(c.max_violation, k) for k, c in enumerate(certs) if c.status == 0]
    print("certificates: %d evaluated, %d without a solution, %d rows each" % (len(ok), len(certs) - len(ok), certs[ok[0][1]].rows if ok else -1))
    if ok:
        v, k = max(ok)
        c = certs[k]
        print("worst violation %.3e: instance %d (seed %d), family A%d, row %d; max objective %.6g, max integrality distance %g"
              % (v, k, a.seed0 + k, c.worst_family, c.worst_row, max(certs[q].objective for _, q in ok), max(certs[q].max_int_infeas for _, q in ok)))
        print("violations above 1e-5: %d" % int(np.sum(np.array([x for x, _ in ok]) > 1e-5)))


if __name__ == "__main__":
    main()

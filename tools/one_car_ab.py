"""A/B of the dual active-set launches against the interior point on one-car shapes (GPU only): MIQP_AS is read per call, so both
modes run in one process, alternating, on the same seeded instances.  python tools/one_car_ab.py [repeats] [out.json]

Per shape (cfg1: the shape of cplexmodel_testcase.dat, cfg2) and mode it prints
  * single solves, seeds 0-95 at gap 0.1 (the planner's call pattern, tools/single_latency.py): latency p50 / p90 / p99 per repeat,
  * the same seeds at gap 1e-7: active-set steps per node against interior point iterations per node,
  * a queue of 256 instances at gap 1e-4 in one batch call: node relaxations of the call per second of the standard launch
    (HIP events around that launch, lastTiming()['std_launch_s']) and per second of the call."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import planner_miqp_amd as P
from planner_miqp_amd import synthetic

SHAPES = {"cfg1": (1, 20, 32, 1, 1), "cfg2": (1, 20, 16, 1, 0)}


def singles(shape, gap, seeds, mode):
    os.environ["MIQP_AS"] = mode
    w = P.CplexWrapper()
    lat = []; tot = dict(nodes=0, iters=0, as_nodes=0, as_steps=0, as_unfinished=0, solved=0)
    for s in seeds:
        w.resetParameters(synthetic.generate(shape, s, gap=gap, max_time=10.0))
        t = time.perf_counter(); st = w.callCplex(); dt = time.perf_counter() - t   # (callCplex returns after the device has finished: it reads the results back)
        pr = w.getSolutionProperties()
        if int(st) == 0 and pr.status in (101, 102):
            tm = w.lastTiming()
            lat.append(dt); tot["solved"] += 1; tot["nodes"] += int(pr.nodes); tot["iters"] += int(pr.NrIterations)
            for k in ("as_nodes", "as_steps", "as_unfinished"):
                tot[k] += tm[k]
    return lat, tot


def queue(shape, mode, n=256, gap=1e-4):
    os.environ["MIQP_AS"] = mode
    ws = []
    for s in range(1000, 1000 + n):
        w = P.CplexWrapper(); w.resetParameters(synthetic.generate(shape, s, gap=gap, max_time=20.0)); ws.append(w)
    P.prepare_batch(ws)
    t = time.perf_counter(); sts = P.solve_batch(ws, prepared=True); dt = time.perf_counter() - t
    tm = ws[0].lastTiming()
    return dict(proven=sum(int(s) == 0 for s in sts), nodes=tm["nodes"], call_s=dt, solve_s=tm["solve_s"], std_launch_s=tm["std_launch_s"], std_launches=tm["std_launches"],
                as_nodes=tm["as_nodes"], as_steps=tm["as_steps"], as_unfinished=tm["as_unfinished"], ipm_iters=tm["ipm_iters"])


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    out = {}
    for name, shape in SHAPES.items():
        for mode in ("1", "0"):   # warm-up: the context of the shape, the code objects of both paths
            singles(shape, 0.1, range(200, 208), mode)
        res = out[name] = {"1": dict(lat=[]), "0": dict(lat=[])}
        for r in range(reps):
            for mode in (("1", "0") if r % 2 == 0 else ("0", "1")):
                lat, tot = singles(shape, 0.1, range(96), mode)
                q = [1e3 * float(np.percentile(lat, x)) for x in (50, 90, 99)]
                res[mode]["lat"].append(q)
                print("%s MIQP_AS=%s gap 0.1 repeat %d: %d of 96 proven, latency ms p50 %.2f p90 %.2f p99 %.2f, %.1f nodes per solve" % (name, mode, r, tot["solved"], q[0], q[1], q[2], tot["nodes"] / max(1, tot["solved"])), flush=True)
        for mode in ("1", "0"):
            lat, tot = singles(shape, 1e-7, range(96), mode)
            res[mode]["tight"] = tot
            if mode == "1":
                print("%s MIQP_AS=1 gap 1e-7: %d nodes, %d by the active-set launches in %d steps = %.2f steps per node, %d returned unsolved; all nodes: %.2f iterations + steps per node"
                      % (name, tot["nodes"], tot["as_nodes"], tot["as_steps"], tot["as_steps"] / max(1, tot["as_nodes"]), tot["as_unfinished"], tot["iters"] / max(1, tot["nodes"])), flush=True)
            else:
                print("%s MIQP_AS=0 gap 1e-7: %d nodes, %.2f interior point iterations per node" % (name, tot["nodes"], tot["iters"] / max(1, tot["nodes"])), flush=True)
        for mode in ("1", "0"):
            queue(shape, mode)
        for r in range(reps):
            for mode in (("1", "0") if r % 2 == 0 else ("0", "1")):
                q = queue(shape, mode)
                res[mode].setdefault("queue", []).append(q)
                print("%s MIQP_AS=%s queue of 256 at 1e-4, repeat %d: %d proven, %d nodes, call %.1f ms, standard launches %d in %.2f ms = %.0f nodes/s of the standard launch, %.0f nodes/s of the call"
                      % (name, mode, r, q["proven"], q["nodes"], 1e3 * q["call_s"], q["std_launches"], 1e3 * q["std_launch_s"], q["nodes"] / max(1e-9, q["std_launch_s"]), q["nodes"] / q["call_s"]), flush=True)
    if len(sys.argv) > 2:
        json.dump(out, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()

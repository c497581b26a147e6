"""The launches of a round do the same work as before they were planned (plan_node_launches / run_node_launches in csrc/miqp_gpu.hip).

The plan and the launcher move no device work: which kernel takes which node, on which counters and lists, is what it was.  So the counts of
a solve are what they were: one callCplex at gap 1e-7 per shape - node relaxations, interior point iterations, the nodes the active-set launches
took and those they could not finish - and one solveFixed of the shape's complete record with the launch of the serial chain that solved it.
Shapes: one car (the <1, ...> kernels and the one-car active-set launches), two cars on three steps and on six with two environment pieces
and a pentagon (the four concurrent launches, class lists), three cars (the memory-backed kernel alone).

tests/golden/launch_plan_counts.json holds the counts of the commit before the plan, recorded on an MI355X; two runs there gave the same
counts, every counter of the list below included.
All tests here need a real MI355X: run with  python -m pytest tests/test_launch_plan_gpu.py -m gpu."""
import json
import os

import pytest

import helpers as H
import planner_miqp_amd as P

pytestmark = pytest.mark.gpu

SHAPES = ["c1n6r16hex", "c2n3", "c2n6e2pent", "mini3"]
GOLDEN = os.path.join(H.GOLDEN, "launch_plan_counts.json")


def counts(oracle, name):
    """the counters of one solve and one solveFixed of NODE_SHAPES[name], each on a handle of its own"""
    p, h, dims, rec = H.node_instance(oracle, name)
    w = P.CplexWrapper(gap_override=1e-7); w.resetParameters(p)
    st = w.callCplex()
    props, t = w.getSolutionProperties(), w.lastTiming()
    f = P.CplexWrapper(); f.resetParameters(p)
    rc = f.solveFixed(rec)[0]
    return dict(status=int(st), nodes=int(props.nodes), iterations=int(props.NrIterations), as_nodes=t["as_nodes"], as_unfinished=t["as_unfinished"],
                fixed_rc=int(rc), fixed_route=f.lastFixedRoute())


@pytest.mark.parametrize("name", SHAPES)
def test_a_solve_does_the_work_it_did_before_the_launches_were_planned(oracle, name):
    want = json.load(open(GOLDEN))[name]
    got = counts(oracle, name)
    print("LAUNCHPLAN %s %s" % (name, json.dumps(got, sort_keys=True)))
    assert got == want, (name, got, want)

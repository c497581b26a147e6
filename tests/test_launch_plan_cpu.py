"""The node launches of a round as plan_node_launches (csrc/miqp_gpu.hip) decides them, through miqp_solver_launch_plan / CplexWrapper.launchPlan:
which kernels run, on which stream, with how many workgroups and how much LDS, on which counters, lists and per-block buffers, behind which memsets.
Host code only: no test here needs a GPU.

The expected rows are written out literally.  They were derived by hand from launch_ipm_batch as it stood before the plan existed (its three shapes:
the serial chain, the probe overlap, the concurrent round), with the capacities ctx_sizes gives a single solve on 256 CUs and 256 GB free: up to
two cars and 20 steps  oc_grid 2048, ocb_grid 1024, probe_grid 1536, ipm_grid_max 3072;  three and four cars  ipm_grid_max 1024 and no on-chip kernel.
For the shapes here the padded LDS of a larger block beside the standard active-set launch (oc_big_lds_beside_as) is the unpadded size: two standard
active-set blocks are smaller than one larger block on these short horizons.

Columns (wrapper.LAUNCH_PLAN_FIELDS): kernel 0 memory-backed, 1 / 2 larger active-set / larger on-chip interior point, 3 / 4 standard active-set / standard on-chip interior point;
stream 0 the solver's, 2 .. 4 beside it; grid; lds; ovf_mode, cls_take, as_split, skip_probes, bounce; work counter (> 0 word of the parity set,
0 the batch's, -1 work_counter2); from_ovf2; bufs (0 primary, 1 second stream's, 2 those with kgain3); zero (1 work counter, 2 ovf_count, 4 ovf2_count).

The shipped library does not read MIQP_CONCURRENT_BIG (a tuning switch), so the export cannot reach the probe overlap through the environment:
launchPlan(concurrent=False) asks for a context without the concurrent round directly."""
import pytest

import helpers as H
import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.wrapper import LAUNCH_PLAN_FIELDS

IPM, AS_BIG, OC_BIG, AS, OC = range(5)
# l_ipm, l_oc, l_ocb (= oc_big_lds_beside_as here), l_as of the shapes with an on-chip kernel
LDS = {"c2n3": (9712, 17008, 30576, 12656), "c1n2r16": (9328, 16800, 30368, 12192)}
LDS_IPM = {"mini3": 15616, "mini4": 25888, "c1n21o": 10960}
IPM_GRID_MAX = {"mini3": 1024, "mini4": 1024, "c1n21o": 3072}
_W = {}


def _wrapper(name):
    if name not in _W:
        cfg, seed, tweaks = H.NODE_SHAPES[name]
        p = synthetic.generate(cfg, seed, gap=1e-7, max_time=30)
        H.tweak_instance(p, **tweaks)
        w = P.CplexWrapper(); w.resetParameters(p)
        _W[name] = w
    return _W[name]


def test_a_row_has_the_documented_columns():
    assert len(LAUNCH_PLAN_FIELDS) == 13 and LAUNCH_PLAN_FIELDS[:4] == ("kernel", "stream", "grid", "lds") and LAUNCH_PLAN_FIELDS[-1] == "zero"


@pytest.mark.parametrize("name", ["mini3", "mini4", "c1n21o"])
@pytest.mark.parametrize("mode", [dict(overlap=0, par=-1), dict(overlap=1, par=-1), dict(overlap=1, par=0), dict(overlap=1, par=1, cls_n=(5, 0, 2))])
def test_a_shape_without_an_on_chip_kernel_has_one_memory_backed_launch(name, mode):
    """(a), (b): three and four cars, and one car beyond 20 steps - one launch on stream 0, grid min(bc, ipm_grid_max), work counter zeroed"""
    for bc in (1, 100, 5000):
        assert _wrapper(name).launchPlan(bc, **mode) == [(IPM, 0, min(bc, IPM_GRID_MAX[name]), LDS_IPM[name], 0, 0, 0, 0, 0, 0, 0, 0, 1)]


@pytest.mark.parametrize("name", ["c2n3", "c1n2r16"])
def test_the_serial_chain_has_three_launches_on_stream_0(name):
    """(c), (h): standard, larger, memory-backed; modes 0, 1, 1; the last reads the ovf2 list; memsets ovf2_count + work_counter + ovf_count, then
    work_counter for each of the other two"""
    l_ipm, l_oc, l_ocb, l_as = LDS[name]
    assert _wrapper(name).launchPlan(1, overlap=0, par=-1) == [
        (OC, 0, 1, l_oc, 0, 0, 0, 0, 0, 0, 0, 0, 7),
        (OC_BIG, 0, 1, l_ocb, 1, 0, 0, 0, 0, 0, 0, 0, 1),
        (IPM, 0, 1, l_ipm, 1, 0, 0, 0, 0, 0, 1, 0, 1)]
    # a polish of many incumbents: each grid capped by its kernel's resident blocks; the active-set switch and the lists change nothing here
    assert _wrapper(name).launchPlan(5000, overlap=0, par=-1, as_on=0, cls_n=(5, 0, 2)) == [
        (OC, 0, 2048, l_oc, 0, 0, 0, 0, 0, 0, 0, 0, 7),
        (OC_BIG, 0, 1024, l_ocb, 1, 0, 0, 0, 0, 0, 0, 0, 1),
        (IPM, 0, 3072, l_ipm, 1, 0, 0, 0, 0, 0, 1, 0, 1)]


@pytest.mark.parametrize("name", ["c2n3", "c1n2r16"])
@pytest.mark.parametrize("par", [0, 1])
def test_the_concurrent_round_has_four_launches_on_four_streams(name, par):
    """(d), (h): larger active-set on stream 3 (word 6, scans the batch), larger interior point on stream 2 (ovf_mode 2, as_split, word 4),
    memory-backed on stream 4 (ovf_mode 3, kgain3, word 5, the larger variant's list), standard active-set on stream 0 (skip_probes, bounce,
    word 1); no memsets"""
    l_ipm, l_oc, l_ocb, l_as = LDS[name]
    assert _wrapper(name).launchPlan(3000, overlap=1, par=par, as_on=1) == [
        (AS_BIG, 3, 1024, l_ocb, 2, 0, 0, 0, 0, 6, 0, 1, 0),
        (OC_BIG, 2, 1024, l_ocb, 2, 0, 1, 0, 0, 4, 0, 1, 0),
        (IPM, 4, 1536, l_ipm, 3, 0, 1, 0, 0, 5, 1, 2, 0),
        (AS, 0, 2048, l_as, 0, 0, 0, 1, 1, 1, 0, 0, 0)]
    # the concurrent form has no batch limit (the probe overlap has: 4096)
    assert [r[:3] for r in _wrapper(name).launchPlan(4097, overlap=1, par=par, as_on=1)] == [(AS_BIG, 3, 1024), (OC_BIG, 2, 1024), (IPM, 4, 1536), (AS, 0, 2048)]


def test_class_lists_size_the_larger_launches_and_an_empty_class_has_no_launch():
    """(e): lists {5, 0, 2} of a round of 100 nodes - gb = 100, share of class 1 = max(32, int(100 * 6 * 5 / (6 * 5 + 93 + 1) + 0.5)) = 32, grid
    min(100, 32, 5) = 5; class 2 is empty: no launch; class 3 min(probe_grid, 2) = 2"""
    l_ipm, l_oc, l_ocb, l_as = LDS["c2n3"]
    assert _wrapper("c2n3").launchPlan(100, overlap=1, par=0, as_on=1, cls_n=(5, 0, 2)) == [
        (AS_BIG, 3, 5, l_ocb, 2, 1, 0, 0, 0, 6, 0, 1, 0),
        (IPM, 4, 2, l_ipm, 3, 3, 1, 0, 0, 5, 1, 2, 0),
        (AS, 0, 100, l_as, 0, 0, 0, 1, 1, 1, 0, 0, 0)]
    # shares above the floor: 3000 nodes, lists {400, 300, 2} - gb = 1024, den = 6 * 400 + 28 * 300 + 2298 + 1 = 13099,
    # class 1 int(1024 * 2400 / 13099 + 0.5) = 188, class 2 min(int(1024 * 8400 / 13099 + 0.5) = 657, 300) = 300
    assert _wrapper("c2n3").launchPlan(3000, overlap=1, par=1, as_on=1, cls_n=(400, 300, 2)) == [
        (AS_BIG, 3, 188, l_ocb, 2, 1, 0, 0, 0, 6, 0, 1, 0),
        (OC_BIG, 2, 300, l_ocb, 2, 2, 1, 0, 0, 4, 0, 1, 0),
        (IPM, 4, 2, l_ipm, 3, 3, 1, 0, 0, 5, 1, 2, 0),
        (AS, 0, 2048, l_as, 0, 0, 0, 1, 1, 1, 0, 0, 0)]
    # every class empty: the standard launch alone, and no stream beside the solver's is touched
    assert _wrapper("c2n3").launchPlan(100, overlap=1, par=0, as_on=1, cls_n=(0, 0, 0)) == [(AS, 0, 100, l_as, 0, 0, 0, 1, 1, 1, 0, 0, 0)]


def test_without_the_active_set_launches_the_round_has_three():
    """(f): the standard launch is the on-chip interior point; the memory-backed kernel follows the larger variant on stream 2 with its list; the
    class lists are not used"""
    l_ipm, l_oc, l_ocb, l_as = LDS["c2n3"]
    want = [(OC_BIG, 2, 1024, l_ocb, 2, 0, 0, 0, 0, 4, 0, 1, 0),
            (IPM, 2, 1536, l_ipm, 1, 0, 0, 0, 0, 5, 1, 1, 0),
            (OC, 0, 2048, l_oc, 0, 0, 0, 1, 1, 1, 0, 0, 0)]
    assert _wrapper("c2n3").launchPlan(3000, overlap=1, par=0, as_on=0) == want
    assert _wrapper("c2n3").launchPlan(3000, overlap=1, par=0, as_on=0, cls_n=(5, 0, 2)) == want


def test_a_round_without_the_parity_counters_zeroes_them_by_memsets():
    """(g): par = -1 - no active-set launches (they come with the parity set); work_counter2 for the launches of stream 2; ovf2_count zeroed ahead of
    everything, each work counter and the standard launch's ovf_count in front of its launch"""
    l_ipm, l_oc, l_ocb, l_as = LDS["c2n3"]
    assert _wrapper("c2n3").launchPlan(3000, overlap=1, par=-1, as_on=1) == [
        (OC_BIG, 2, 1024, l_ocb, 2, 0, 0, 0, 0, -1, 0, 1, 5),
        (IPM, 2, 1536, l_ipm, 1, 0, 0, 0, 0, -1, 1, 1, 1),
        (OC, 0, 2048, l_oc, 0, 0, 0, 1, 1, 0, 0, 0, 3)]


def test_the_probe_overlap_stops_at_4096_nodes():
    """(i): a context without the concurrent round - up to 4096 nodes the larger variant takes the probes on stream 2 beside the standard launch
    (which skips them, without bounce), then the chain; beyond, the chain alone"""
    l_ipm, l_oc, l_ocb, l_as = LDS["c2n3"]
    chain = [(OC_BIG, 0, 1024, l_ocb, 1, 0, 0, 0, 0, 0, 0, 0, 1), (IPM, 0, 3072, l_ipm, 1, 0, 0, 0, 0, 0, 1, 0, 1)]
    assert _wrapper("c2n3").launchPlan(4096, overlap=1, par=0, as_on=1, concurrent=False) == [
        (OC_BIG, 2, 1024, l_ocb, 2, 0, 0, 0, 0, -1, 0, 1, 5),
        (OC, 0, 2048, l_oc, 0, 0, 0, 1, 0, 0, 0, 0, 3)] + chain
    assert _wrapper("c2n3").launchPlan(4097, overlap=1, par=0, as_on=1, concurrent=False) == [(OC, 0, 2048, l_oc, 0, 0, 0, 0, 0, 0, 0, 0, 7)] + chain
    assert _wrapper("c2n3").launchPlan(4096, overlap=0, par=-1, concurrent=False) == [(OC, 0, 2048, l_oc, 0, 0, 0, 0, 0, 0, 0, 0, 7)] + chain

"""Which shapes have the dual active-set launches (as_shape_ok in csrc/as_onchip.hip, exported as miqp_gpu_has_active_set and
planner_miqp_amd.has_active_set): one or two cars with a horizon of up to 20 steps.  Host code only: no test here needs a GPU."""
import os
import re

import pytest

import planner_miqp_amd as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


@pytest.mark.parametrize("cars,steps,want", [(1, 20, 1), (1, 2, 1), (2, 20, 1), (2, 2, 1),
                                             (1, 21, 0), (2, 21, 0), (1, 40, 0), (3, 10, 0), (4, 10, 0), (0, 10, 0), (5, 6, 0), (1, 0, 0), (-1, 10, 0)])
def test_has_active_set_says_which_shapes_have_the_launches(lib, cars, steps, want):
    assert P.has_active_set(cars, steps) == want
    assert lib.miqp_gpu_has_active_set(cars, steps) == want


def test_the_library_exports_the_predicate_and_the_header_declares_it(lib):
    assert hasattr(lib, "miqp_gpu_has_active_set")
    from planner_miqp_amd.wrapper import EXPORTED_SYMBOLS
    assert "miqp_gpu_has_active_set" in EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "miqp_gpu.h")).read()
    assert re.search(r"\bint\s+miqp_gpu_has_active_set\s*\(\s*int\s+num_cars\s*,\s*int\s+num_steps\s*\)\s*;", hdr)


def test_one_predicate_decides_every_site_of_the_host_code():
    """the car count of the launches is asked in one place: no `Y.C == 2` is left at the capacities, the launches, the LDS attributes
    or the ring (the round width of plan_call and the two-car cost map of the diagnostics are other questions)"""
    src = open(os.path.join(ROOT, "planner_miqp_amd", "csrc", "miqp_gpu.hip")).read()
    left = [ln.strip() for ln in src.split("\n") if re.search(r"\bC == 2\b", ln) and "round_nodes" not in ln]
    assert left == [], left
    assert src.count("as_shape_ok(") >= 5
    kern = open(os.path.join(ROOT, "planner_miqp_amd", "csrc", "as_onchip.hip")).read()
    assert len(re.findall(r"constexpr bool as_shape_ok\(int C, int N\)", kern)) == 1
    # the four instantiations of the active-set kernel are named in the kernel table, which the launcher and set_kernel_lds read, and nowhere else
    table = src[src.index("const NodeKernelFn NODE_KERNEL["):]
    table = table[:table.index("};")]
    for c in (1, 2):
        for spelling in ("as_onchip_kernel<%d, OC_NSL>" % c, "as_onchip_kernel<%d, OC_NSL, OC_GCAP_BIG>" % c):
            assert spelling in table and src.count(spelling) == 1, spelling

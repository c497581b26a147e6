"""Starts from the carried pool (miqp_solver_set_pool_starts, miqp_solver_pool_starts_last), as far as it can be checked without a
device: the exports, the header's text, the bindings and the C++ wrapper's methods; the refusals; the wrapper's side of the setting across
resetParameters - read back from the library with miqp_solver_get_pool_starts -; the empty answer of a handle that has not solved; and that the
feature brought no second copy of a capture kernel or of eval_kernel.  What a solve does with the setting is in test_pool_starts_gpu.py."""
import ctypes as C
import glob
import os
import re

import pytest

import planner_miqp_amd as P
from test_pool_carry_cpu import _loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def test_the_exports_exist_and_bind(lib):
    hdr = open(os.path.join(ROOT, "include", "miqp_gpu.h")).read()
    for n in ("miqp_solver_set_pool_starts", "miqp_solver_pool_starts_last", "miqp_solver_get_pool_starts"):
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS
        assert getattr(lib, n).restype is C.c_int and getattr(lib, n).argtypes
    assert len(lib.miqp_solver_set_pool_starts.argtypes) == 2 and len(lib.miqp_solver_pool_starts_last.argtypes) == 3 and len(lib.miqp_solver_get_pool_starts.argtypes) == 1
    assert re.search(r"\bint\s+miqp_solver_get_pool_starts\s*\(\s*const\s+miqp_solver_t\s*\*\s*s\s*\)", hdr)
    assert re.search(r"\bint\s+miqp_solver_set_pool_starts\s*\(\s*miqp_solver_t\s*\*\s*s\s*,\s*int\s+max_starts\s*\)", hdr)
    assert re.search(r"\bint\s+miqp_solver_pool_starts_last\s*\(\s*const\s+miqp_solver_t\s*\*\s*s\s*,\s*int\s*\*\s*place\s*,\s*int\s+cap\s*\)", hdr)
    # what the setting does and where it does not apply is said where it is declared; the carry no longer lists the starts as out of scope
    for text in ("TAKES STARTS", "survives", "tree-split call", "IGNORES the setting", "No kernel is added or changed", "depth word 0", "needs no device"):
        assert text in hdr, text
    assert "that would change solves" not in hdr
    src = open(os.path.join(ROOT, "planner_miqp_amd", "csrc", "pool_carry.hip")).read()
    assert "that would change solves" not in src and "miqp_solver_set_pool_starts" in src
    assert callable(P.CplexWrapper.setSolutionPoolStarts) and callable(P.CplexWrapper.solutionPoolStartsLast)
    cpp = open(os.path.join(ROOT, "include", "cplex_wrapper.hpp")).read()
    assert re.search(r"\bint\s+setSolutionPoolStarts\s*\(\s*int\s+max_starts\s*\)", cpp)
    assert re.search(r"std::vector<int>\s+solutionPoolStartsLast\s*\(\s*\)\s*const", cpp)
    assert "miqp_solver_set_pool_starts(h_" in cpp and "miqp_solver_pool_starts_last(h_" in cpp
    # the C++ class loads its parameters inside callCplex only: it says where it is declared that no solve takes a start through it alone
    assert "THROUGH THIS CLASS ALONE NO SOLVE TAKES A START" in cpp and "keepLoaded_" not in cpp


def test_refusals_keep_the_old_setting(lib):
    f = lib.miqp_solver_set_pool_starts
    top = P.pool_max()
    assert top == 16
    assert f(None, 1) == -1 and lib.miqp_solver_pool_starts_last(None, None, 0) == -1
    assert lib.miqp_solver_get_pool_starts(None) == -1
    w = P.CplexWrapper()
    assert w.solutionPoolStarts() == 0   # off by default
    assert w.setSolutionPoolStarts(5) == 0 and w._starts == 5 and w.solutionPoolStarts() == 5
    for bad in (-1, -7, top + 1, 1000):
        assert w.setSolutionPoolStarts(bad) == -1 and w._starts == 5 and w.solutionPoolStarts() == 5, bad
        assert f(w._h, bad) == -1 and w.solutionPoolStarts() == 5, bad
    for good in (0, 1, top):
        assert w.setSolutionPoolStarts(good) == 0 and w._starts == good and w.solutionPoolStarts() == good
    # a place array may be absent when none is asked for
    assert lib.miqp_solver_pool_starts_last(w._h, None, 0) == 0


def test_the_setting_survives_new_parameters_and_a_handle_without_a_solve_has_no_starts(lib):
    assert P.CplexWrapper().solutionPoolStartsLast() == []
    w = _loaded()
    assert w.setSolutionPool(8) == 0 and w.setSolutionPoolFilter(12) == 0 and w.setSolutionPoolStarts(16) == 0
    assert w.solutionPoolStartsLast() == []
    assert w.solutionPoolStarts() == 16
    w.resetParameters(w._params)
    assert w._push_inputs() == 0   # (miqp_solver_set_params)
    assert w.solutionPoolStarts() == 16 and w._starts == 16 and w.solutionPoolStartsLast() == [] and w.solutionPoolCount() == 0
    # ... as capacity and filter do, and a .dat load as well
    dat = os.path.join(ROOT, "tests", "golden", "ref_data", "cplexmodel_testcase.dat")
    assert lib.miqp_solver_load_dat(w._h, dat.encode()) == 0 and w.solutionPoolStarts() == 16
    # the places are written only as far as the count goes
    place = (C.c_int * 4)(7, 7, 7, 7)
    assert lib.miqp_solver_pool_starts_last(w._h, place, 4) == 0 and list(place) == [7, 7, 7, 7]
    # without a carried pool the wrapper loads its parameters at every solve, as ever
    assert w._keep_loaded is False


def test_no_kernel_was_added():
    """the starts are host code: one definition each of the capture kernels and of eval_kernel (its head is written twice, under the two branches of
    one #if), and select_kernel"""
    src = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "planner_miqp_amd", "csrc", "*"))))
    assert len(re.findall(r"__global__[^\n]*\bvoid\s+pool_merge_kernel\b", src)) == 1
    assert len(re.findall(r"__global__[^\n]*\bvoid\s+pool_filter_kernel\b", src)) == 1
    assert len(re.findall(r"__global__[^\n]*\bselect_kernel\b", src)) == 1
    heads = r"#if MIQP_EVAL_WPE > 0\n__global__[^\n]*\beval_kernel\(DevBuf B\) \{\n#else\n__global__[^\n]*\beval_kernel\(DevBuf B\) \{\n#endif\n"
    assert len(re.findall(heads, src)) == 1 and len(re.findall(r"__global__[^\n]*\beval_kernel\b", src)) == 2
    assert len(re.findall(r"__global__[^\n]*\bstart", src)) == 0

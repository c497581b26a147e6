"""The manoeuvre filter of the solution pool (miqp_solver_set_pool_filter, miqp_gpu_pool_signature, miqp_solver_pool_signature,
miqp_solver_pool_found_decisions), as far as it can be checked without a device: the exports, the setting, every answer that is decided before a
device is asked for, and the signature function against a restatement of its definition.  What the device keeps: test_pool_filter_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import RawResults

NAMES = ("miqp_solver_set_pool_filter", "miqp_gpu_pool_signature", "miqp_solver_pool_signature", "miqp_solver_pool_found_decisions")
DIMS = [(1, 2, 0), (2, 6, 1), (2, 20, 4), (3, 6, 0), (4, 6, 2)]   # (cars, steps, obstacles)
BP = C.POINTER(C.c_byte)


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def _loaded():
    w = P.CplexWrapper(); w.resetParameters(synthetic.generate("mini", 0))
    assert w._push_inputs() == 0
    return w


def _layout(Cn, N, O):
    NP = Cn * (Cn - 1) // 2
    f_env = Cn * N
    f_obs = f_env + 5 * Cn * N
    f_c2c = f_obs + 5 * Cn * O * N
    return f_env, f_obs, f_c2c, f_c2c + 4 * NP * N, NP


def _sites(Cn, N, O):
    """(family bit, [byte position of step i for i in 0 .. N - 1]) of every site, from the layout of the definition"""
    f_env, f_obs, f_c2c, D, NP = _layout(Cn, N, O)
    out = []
    for c in range(Cn):
        out.append((1, [c * N + i for i in range(N)]))
    for c in range(Cn):
        for pt in range(5):
            out.append((2, [f_env + (c * N + i) * 5 + pt for i in range(N)]))
    for c in range(Cn):
        for o in range(O):
            for pt in range(5):
                out.append((4, [f_obs + ((c * O + o) * N + i) * 5 + pt for i in range(N)]))
    for p in range(NP):
        for g in range(4):
            out.append((8, [f_c2c + (p * N + i) * 4 + g for i in range(N)]))
    return out


def _signature(Cn, N, O, families, d):
    """the definition, restated: per site of a selected family the values of steps 1 .. N - 1 that are not negative (a region byte >> 2), repeats
    collapsed, left-packed from step 1; with the timing bit the site's bytes as they are"""
    D = _layout(Cn, N, O)[3]
    s = np.full(D, -1, dtype=np.int8)
    for bit, pos in _sites(Cn, N, O):
        if not families & bit:
            continue
        if families & 16:
            for q in pos:
                s[q] = d[q]
            continue
        seq = []
        for i in range(1, N):
            v = int(d[pos[i]])
            if v < 0:
                continue
            if bit == 1:
                v >>= 2
            if not seq or seq[-1] != v:
                seq.append(v)
        for k, v in enumerate(seq):
            s[pos[1 + k]] = v
    return s


def test_the_exports_exist(lib):
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS
    assert (P.POOL_BY_REGION, P.POOL_BY_ENVIRONMENT, P.POOL_BY_OBSTACLE, P.POOL_BY_CAR_CAR, P.POOL_EXACT_TIMING) == (1, 2, 4, 8, 16)


def test_set_pool_filter_refuses_what_is_out_of_range(lib):
    w = _loaded()
    assert lib.miqp_solver_set_pool_filter(None, 12) == -1
    assert lib.miqp_solver_set_pool_filter(w._h, 0) == 0 and lib.miqp_solver_set_pool_filter(w._h, 31) == 0
    assert lib.miqp_solver_set_pool_filter(w._h, -1) == -2 and lib.miqp_solver_set_pool_filter(w._h, 32) == -2
    assert w.setSolutionPoolFilter(12) == 0 and w.setSolutionPoolFilter(32) == -2 and w.setSolutionPoolFilter(-1) == -2
    assert w.setSolutionPoolFilter(P.POOL_BY_OBSTACLE | P.POOL_BY_CAR_CAR) == lib.miqp_solver_set_pool_filter(w._h, 12) == 0
    assert w.setSolutionPoolFilter(0) == 0


@pytest.mark.parametrize("dims", DIMS)
def test_the_signature_is_the_definition(lib, dims):
    """random records with bytes in -1 .. 7, step-0 bytes random too, every families value: the library's bytes are those of the restatement above"""
    Cn, N, O = dims
    D = _layout(Cn, N, O)[3]
    assert D == P.wrapper._decision_len(Cn, N, O)
    rng = np.random.default_rng(1000 * Cn + 10 * N + O)
    for rep in range(6):
        d = rng.integers(-1, 8, size=D).astype(np.int8)
        if rep == 5:   # long runs of one value, so that collapsing has something to collapse
            d = np.repeat(rng.integers(-1, 8, size=(D + 2) // 3), 3)[:D].astype(np.int8)
        keep = d.copy()
        for fam in range(1, 32):
            got = P.pool_signature(Cn, N, O, fam, d)
            want = _signature(Cn, N, O, fam, d)
            assert got.dtype == np.int8 and got.shape == (D,)
            assert np.array_equal(got, want), (dims, fam, rep, np.nonzero(got != want)[0][:8])
        assert np.array_equal(d, keep)


@pytest.mark.parametrize("dims", DIMS)
def test_all_families_with_exact_timing_is_the_record(lib, dims):
    Cn, N, O = dims
    D = _layout(Cn, N, O)[3]
    d = np.random.default_rng(7).integers(-1, 8, size=D).astype(np.int8)
    assert P.pool_signature(Cn, N, O, 31, d).tobytes() == d.tobytes()


def _record(Cn, N, O):
    """a decided record: every byte 0"""
    return np.zeros(_layout(Cn, N, O)[3], dtype=np.int8)


def test_the_step_of_a_switch_is_timing_the_order_is_not(lib):
    """two cars, six steps, one obstacle; group 0 of the pair switches from alternative 1 to alternative 2 - at step 3 in one record, at step 4 in the
    other: one manoeuvre under car/car (8), two under car/car with exact timing (24).  A third record switches from 2 to 1: another order, another
    manoeuvre under 8"""
    Cn, N, O = 2, 6, 1
    f_c2c = _layout(Cn, N, O)[2]
    a, b, c = _record(Cn, N, O), _record(Cn, N, O), _record(Cn, N, O)
    for i in range(N):
        a[f_c2c + i * 4] = 1 if i < 3 else 2
        b[f_c2c + i * 4] = 1 if i < 4 else 2
        c[f_c2c + i * 4] = 2 if i < 3 else 1
    sa, sb, sc = (P.pool_signature(Cn, N, O, 8, x) for x in (a, b, c))
    assert np.array_equal(sa, sb)
    assert not np.array_equal(P.pool_signature(Cn, N, O, 24, a), P.pool_signature(Cn, N, O, 24, b))
    assert not np.array_equal(sa, sc)
    # the sequence itself, left-packed from step 1: 1, 2, then nothing
    assert [int(sa[f_c2c + i * 4]) for i in range(N)] == [-1, 1, 2, -1, -1, -1]
    # ... and the same three records do not differ under a family they agree in
    assert np.array_equal(P.pool_signature(Cn, N, O, 4, a), P.pool_signature(Cn, N, O, 4, c))


def test_a_region_byte_counts_by_its_region_and_step_0_is_not_read(lib):
    Cn, N, O = 1, 4, 0
    a, b = _record(Cn, N, O), _record(Cn, N, O)
    a[0:4] = [9, 4, 5, 8]    # regions -, 1, 1, 2 (the low two bits are the half-plane)
    b[0:4] = [0, 6, 8, 11]   # regions -, 1, 2, 2
    sa, sb = P.pool_signature(Cn, N, O, 1, a), P.pool_signature(Cn, N, O, 1, b)
    assert np.array_equal(sa, sb) and list(sa[0:4]) == [-1, 1, 2, -1]
    assert not np.array_equal(P.pool_signature(Cn, N, O, 17, a), P.pool_signature(Cn, N, O, 17, b))


def test_the_error_codes_of_the_byte_function(lib):
    d = np.zeros(64, dtype=np.int8); o = np.zeros(64, dtype=np.int8)
    dp, op = d.ctypes.data_as(BP), o.ctypes.data_as(BP)
    f = lib.miqp_gpu_pool_signature
    assert f(1, 2, 0, 12, dp, op, 64) == 12      # D of one car, two steps
    assert f(1, 2, 0, 12, dp, op, 12) == 12
    assert f(1, 2, 0, 12, None, op, 64) == -1 and f(1, 2, 0, 12, dp, None, 64) == -1
    assert f(0, 2, 0, 12, dp, op, 64) == -1 and f(1, 0, 0, 12, dp, op, 64) == -1 and f(1, 2, -1, 12, dp, op, 64) == -1
    assert f(1, 2, 0, 0, dp, op, 64) == -2 and f(1, 2, 0, 32, dp, op, 64) == -2 and f(1, 2, 0, -1, dp, op, 64) == -2
    assert f(1, 2, 0, 12, dp, op, 11) == -3
    with pytest.raises(ValueError):
        P.pool_signature(1, 2, 0, 0, d[:12])
    with pytest.raises(ValueError):
        P.pool_signature(1, 2, 0, 12, d[:11])


def test_the_error_codes_on_a_handle(lib):
    w = _loaded()
    dims = (C.c_int * 6)()
    assert lib.miqp_solver_get_dims(w._h, dims) == 0
    D = P.wrapper._decision_len(dims[0], dims[1], dims[4])
    r = RawResults(*list(dims))
    o = np.zeros(D, dtype=np.int8); op = o.ctypes.data_as(BP)
    f = lib.miqp_solver_pool_signature
    assert f(w._h, C.byref(r.to_c()), 12, op, D) == D
    assert f(None, C.byref(r.to_c()), 12, op, D) == -1 and f(w._h, None, 12, op, D) == -1 and f(w._h, C.byref(r.to_c()), 12, None, D) == -1
    assert f(P.CplexWrapper()._h, C.byref(r.to_c()), 12, op, D) == -1      # a handle without an instance
    assert f(w._h, C.byref(r.to_c()), 0, op, D) == -2 and f(w._h, C.byref(r.to_c()), 32, op, D) == -2
    other = RawResults(dims[0], dims[1] + 1, dims[2], dims[3], dims[4], dims[5])
    assert f(w._h, C.byref(other.to_c()), 12, op, D) == -3
    assert f(w._h, C.byref(r.to_c()), 12, op, D - 1) == -4
    # an all-zero record asserts nothing: every disjunction takes its first alternative or stays open, and the wrapper hands out D bytes
    s = w.poolSignature(r, 12)
    assert s.dtype == np.int8 and s.shape == (D,)
    with pytest.raises(ValueError):
        w.poolSignature(r, 0)
    # a handle without a pool has no entry to hand out
    g = lib.miqp_solver_pool_found_decisions
    assert g(w._h, 0, op, D) == -1 and g(None, 0, op, D) == -1 and g(w._h, 0, None, D) == -1 and g(w._h, -1, op, D) == -1
    assert w.setSolutionPool(8) == 0 and g(w._h, 0, op, D) == -1          # pool on, no solve
    assert w.solutionPoolFoundDecisions(0) is None


def test_the_wrapper_methods_forward(lib):
    w = _loaded()
    for n in ("setSolutionPoolFilter", "solutionPoolFoundDecisions", "poolSignature"):
        assert callable(getattr(w, n)), n
    assert callable(P.pool_signature)

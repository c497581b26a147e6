"""The climb of the solution pool inside its manoeuvre classes (miqp_gpu_pool_moves, miqp_solver_solve_decisions, miqp_solver_pool_improve), as far as
it can be checked without a device: the exports, the neighbourhood against a restatement of its definition, the binding check and every
answer that is decided before a device is asked for.  What the device does: test_pool_improve_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import PoolImproveC
from test_pool_filter_cpu import DIMS, _layout, _sites

NAMES = ("miqp_gpu_pool_moves", "miqp_gpu_pool_moves_max", "miqp_gpu_pool_improve_size", "miqp_solver_solve_decisions", "miqp_solver_pool_improve")
BP, IP = C.POINTER(C.c_byte), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def _loaded():
    w = P.CplexWrapper(); w.resetParameters(synthetic.generate("mini", 0))
    assert w._push_inputs() == 0
    return w


def _site_sequence(bit, b):
    """the timing-free signature of one site, restated: the decided values of steps 1 .. N - 1 (a region byte >> 2), repeats collapsed"""
    seq = []
    for v in b[1:]:
        v = int(v)
        if v < 0:
            continue
        if bit == 1:
            v >>= 2
        if not seq or seq[-1] != v:
            seq.append(v)
    return seq


def _candidates(Cn, N, O, families, d):
    """the definition, restated: (kept, (first, stride, count, value)) of every candidate move in the order site, change point, L1 L2 E1 E2"""
    out = []
    for bit, pos in _sites(Cn, N, O):
        b = [int(d[q]) for q in pos]
        stride = pos[1] - pos[0]
        for i in range(2, N):
            if b[i] == b[i - 1] or b[i] < 0 or b[i - 1] < 0:
                continue
            cand = [(i, 1, b[i - 1])]
            if i + 1 < N:
                cand.append((i, 2, b[i - 1]))
            cand.append((i - 1, 1, b[i]))
            if i - 2 >= 1:
                cand.append((i - 2, 2, b[i]))
            for i0, cnt, v in cand:
                nb = list(b)
                for k in range(cnt):
                    nb[i0 + k] = v
                kept = not (families & bit) or _site_sequence(bit, nb) == _site_sequence(bit, b)
                out.append((kept, (pos[i0], stride, cnt, v)))
    return out


def _apply(d, mv):
    n = np.array(d, dtype=np.int8)
    for k in range(mv[2]):
        n[mv[0] + k * mv[1]] = mv[3]
    return n


def test_the_exports_exist(lib):
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS
    assert P.pool_moves_max() == lib.miqp_gpu_pool_moves_max() == 512


def test_the_struct_is_the_librarys(lib):
    assert lib.miqp_gpu_pool_improve_size() == C.sizeof(PoolImproveC) == 24
    assert [n for n, _ in PoolImproveC._fields_] == ["before", "after", "moves", "status"]


@pytest.mark.parametrize("dims", DIMS)
def test_the_moves_are_the_definition(lib, dims):
    """random records with bytes in -1 .. 7 (step 0 too), one of them with long runs, every families value 1 .. 15: the library's moves are the kept
    candidates of the restatement in its order, cut at pool_moves_max(); every returned move leaves pool_signature unchanged and every dropped
    candidate changes it"""
    Cn, N, O = dims
    D = _layout(Cn, N, O)[3]
    rng = np.random.default_rng(7000 + 1000 * Cn + 10 * N + O)
    recs = [rng.integers(-1, 8, size=D).astype(np.int8), np.repeat(rng.integers(-1, 8, size=(D + 2) // 3), 3)[:D].astype(np.int8)]
    cut = False
    for d in recs:
        for fam in range(1, 16):
            cand = _candidates(Cn, N, O, fam, d)
            want = [mv for kept, mv in cand if kept]
            cut = cut or len(want) > P.pool_moves_max()
            got = P.pool_moves(Cn, N, O, fam, d)
            assert got.dtype == np.int32 and got.shape == (min(len(want), P.pool_moves_max()), 4)
            assert [tuple(int(x) for x in r) for r in got] == want[:P.pool_moves_max()], (dims, fam)
            sig = P.pool_signature(Cn, N, O, fam, d).tobytes()
            for kept, mv in cand:
                assert all(mv[0] + k * mv[1] < D for k in range(mv[2]))
                assert (P.pool_signature(Cn, N, O, fam, _apply(d, mv)).tobytes() == sig) == kept, (dims, fam, mv, kept)
    if dims == (2, 20, 4):
        assert cut   # (a condition on the inputs: this shape's records have more kept moves than the cap, so the cut is exercised)


def test_step_zero_is_never_written_and_values_come_from_the_site():
    Cn, N, O = 2, 20, 4
    D = _layout(Cn, N, O)[3]
    d = np.random.default_rng(5).integers(-1, 8, size=D).astype(np.int8)
    step0 = {pos[0] for _, pos in _sites(Cn, N, O)}
    where = {q: (s, i) for s, (_, pos) in enumerate(_sites(Cn, N, O)) for i, q in enumerate(pos)}
    for first, stride, count, value in P.pool_moves(Cn, N, O, 12, d):
        for k in range(count):
            assert first + k * stride not in step0
        s, i = where[first]
        pos = _sites(Cn, N, O)[s][1]
        assert stride == pos[1] - pos[0] and value in (d[pos[i - 1]], d[pos[min(i + count, N - 1)]])


def _one_site(N, b, fam):
    """the moves of a one-car record whose region site holds b (every other byte undecided), under fam"""
    D = _layout(1, N, 0)[3]
    d = np.full(D, -1, dtype=np.int8)
    d[:N] = b
    return [tuple(int(x) for x in r) for r in P.pool_moves(1, N, 0, fam, d)]


def test_hand_written_records():
    # region bytes 4 q + h: 0, 4, 8 are three regions; 0 and 1 one region with two half-plane alternatives
    # a run of length 1 in the middle (N = 6: steps 1 .. 5 = 0 0 4 8 8): swallowing the 4 changes the signature of a selected family
    b = [-1, 0, 0, 4, 8, 8]
    sel = _one_site(6, b, 1)
    # change point 3 (0 -> 4): L1 swallows the 4 (dropped), L2 too (dropped), E1 (kept), E2: i - 2 = 1 >= 1 swallows the run of 0 (dropped)
    # change point 4 (4 -> 8): L1 (kept), L2 swallows the run of 8 (dropped), E1 swallows the 4 (dropped), E2 too (dropped)
    assert sel == [(2, 1, 1, 4), (4, 1, 1, 4)], sel
    unsel = _one_site(6, b, 2)   # the region family is not selected: every candidate stays
    assert unsel == [(3, 1, 1, 0), (3, 1, 2, 0), (2, 1, 1, 4), (1, 1, 2, 4), (4, 1, 1, 4), (4, 1, 2, 4), (3, 1, 1, 8), (2, 1, 2, 8)], unsel
    # the same region with another half-plane alternative is one value of the region signature: moves between 0 and 1 are all kept
    assert _one_site(6, [-1, 0, 0, 1, 1, 1], 1) == [(3, 1, 1, 0), (3, 1, 2, 0), (2, 1, 1, 1), (1, 1, 2, 1)]
    # change point at i = 2: no E2 (it would write step 0); at i = N - 1: no L2
    assert _one_site(6, [-1, 0, 4, 4, 4, 4], 2) == [(2, 1, 1, 0), (2, 1, 2, 0), (1, 1, 1, 4)]
    assert _one_site(6, [-1, 0, 0, 0, 0, 4], 2) == [(5, 1, 1, 0), (4, 1, 1, 4), (3, 1, 2, 4)]
    # a change at step 1 is no change point (i starts at 2), an undecided neighbour is none either
    assert _one_site(6, [0, 4, 4, 4, 4, 4], 2) == [] and _one_site(6, [-1, 0, -1, 4, -1, 8], 2) == []
    # N = 3: one possible change point, i = 2 = N - 1: L1 and E1 only; under the selected family both swallow a run
    assert _one_site(3, [-1, 0, 4], 2) == [(2, 1, 1, 0), (1, 1, 1, 4)]
    assert _one_site(3, [-1, 0, 4], 1) == []
    assert _one_site(2, [-1, 0], 2) == []


def test_error_codes(lib):
    Cn, N, O = 2, 6, 1
    D = _layout(Cn, N, O)[3]
    d = np.random.default_rng(3).integers(0, 4, size=D).astype(np.int8)
    out = np.zeros((512, 4), dtype=np.int32)
    dp, op = d.ctypes.data_as(BP), out.ctypes.data_as(IP)
    n = lib.miqp_gpu_pool_moves(Cn, N, O, 12, dp, op, 512)
    assert n > 1
    assert lib.miqp_gpu_pool_moves(Cn, N, O, 12, None, op, 512) == -1 and lib.miqp_gpu_pool_moves(Cn, N, O, 12, dp, None, 512) == -1
    assert lib.miqp_gpu_pool_moves(0, N, O, 12, dp, op, 512) == -1 and lib.miqp_gpu_pool_moves(Cn, 0, O, 12, dp, op, 512) == -1
    assert lib.miqp_gpu_pool_moves(Cn, N, -1, 12, dp, op, 512) == -1
    for fam in (0, 16, 28, 31, 32, -1):
        assert lib.miqp_gpu_pool_moves(Cn, N, O, fam, dp, op, 512) == -2, fam
    assert lib.miqp_gpu_pool_moves(Cn, N, O, 12, dp, op, n - 1) == -3 and lib.miqp_gpu_pool_moves(Cn, N, O, 12, dp, op, n) == n
    for fam in (0, 16, 31):
        with pytest.raises(ValueError):
            P.pool_moves(Cn, N, O, fam, d)
    with pytest.raises(ValueError):
        P.pool_moves(Cn, N, O, 12, d[:-1])


def test_improve_answers_before_any_device(lib):
    """the filter and the number of passes are checked first; a handle whose pool is empty returns 0 without touching a device; the pool is as before"""
    w = _loaded()
    assert w.setSolutionPool(8) == 0
    out = (PoolImproveC * 8)()
    assert lib.miqp_solver_pool_improve(None, 8, out, 8) == -1 and lib.miqp_solver_pool_improve(w._h, 8, None, 8) == -1
    assert lib.miqp_solver_pool_improve(w._h, 8, out, 0) == -1
    for fam in (0, 16, 31):
        assert w.setSolutionPoolFilter(fam) == 0
        rc, before, after, moves, status = w.improveSolutionPool()
        assert rc == -2 and len(before) == len(after) == len(moves) == len(status) == 0, (fam, rc)
        assert w.solutionPoolCount() == 0 and len(w.solutionPoolFound()) == 0
    assert w.setSolutionPoolFilter(12) == 0
    for passes in (0, -1, 65):
        assert w.improveSolutionPool(passes)[0] == -2, passes
    import torch
    rc = w.improveSolutionPool()[0]
    assert rc == 0   # (no solve yet: the pool is empty, with or without a device)
    assert w.solutionPoolCount() == 0 and w.solutionPoolFoundDecisions(0) is None
    if not torch.cuda.is_available():
        assert w.callCplex() != P.OptimizationStatus.SUCCESS and w.improveSolutionPool()[0] == 0 and w.solutionPoolCount() == 0
    fresh = P.CplexWrapper()
    assert lib.miqp_solver_pool_improve(fresh._h, 8, out, 8) == -1   # no instance


def test_solve_decisions_without_a_device(lib):
    import torch
    w = _loaded()
    d = (C.c_int * 6)()
    assert lib.miqp_solver_get_dims(w._h, d) == 0
    D = P.wrapper._decision_len(d[0], d[1], d[4])
    rec = np.full((3, D), -1, dtype=np.int8)
    out = (P.FixedResultC * 3)()
    assert lib.miqp_solver_solve_decisions(None, rec.ctypes.data_as(BP), 3, out, None) == -1
    assert lib.miqp_solver_solve_decisions(w._h, None, 3, out, None) == -1 and lib.miqp_solver_solve_decisions(w._h, rec.ctypes.data_as(BP), 0, out, None) == -1
    assert lib.miqp_solver_solve_decisions(w._h, rec.ctypes.data_as(BP), 65537, out, None) == -5
    bad = rec.copy(); bad[:, 1] = 127   # no car has that many possible regions: refused on the host, no device is asked for
    rc, status, obj, viol, it, route, best = w.solveDecisions(bad)
    assert rc == 0 and list(status) == [2, 2, 2] and best == -1 and np.isnan(obj).all() and list(route) == [-1, -1, -1]
    with pytest.raises(ValueError):
        w.solveDecisions(rec[:, :-1])
    if not torch.cuda.is_available():
        rc, status, obj, viol, it, route, best = w.solveDecisions(rec)
        assert rc == -3 and list(status) == [2, 2, 2] and best == -1 and np.isnan(obj).all()

"""The step of the solution pool across manoeuvre classes (miqp_gpu_pool_jumps, miqp_solver_pool_explore), as far as it can be checked without a
device: the exports, the neighbourhood against a restatement of its definition, the binding check and every answer that is decided
before a device is asked for.  What the device does: test_pool_explore_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import planner_miqp_amd as P
from planner_miqp_amd import synthetic
from planner_miqp_amd.ctypes_types import PoolExploreC
from test_pool_filter_cpu import DIMS, _layout, _sites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("miqp_gpu_pool_jumps", "miqp_gpu_pool_explore_size", "miqp_solver_pool_explore")
BP, IP = C.POINTER(C.c_byte), C.POINTER(C.c_int)
LINES = 4   # edges of an obstacle in the random records: bytes 0 .. 3 are edges, 4 is the soft alternative


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def _loaded():
    w = P.CplexWrapper(); w.resetParameters(synthetic.generate("mini", 0))
    assert w._push_inputs() == 0
    return w


def _collapsed(b):
    """the timing-free signature of an obstacle or car/car site, restated: the decided values of steps 1 .. N - 1, repeats collapsed"""
    seq = []
    for v in b[1:]:
        if v >= 0 and (not seq or seq[-1] != v):
            seq.append(v)
    return seq


def _units(Cn, N, O, L, families):
    """(alternatives, [[byte positions of step i] for i in 0 .. N - 1], stride of the move) of every unit that can jump, in the order of the
    definition: obstacle groups by c * O + o, pairs, then the obstacle and car/car sites in pool_site order"""
    f_env, f_obs, f_c2c, D, NP = _layout(Cn, N, O)
    out = []
    if families & 4:
        for g in range(Cn * O):
            out.append((L, [[f_obs + (g * N + i) * 5 + pt for pt in range(5)] for i in range(N)], 1))
    if families & 8:
        for p in range(NP):
            out.append((4, [[f_c2c + (p * N + i) * 4 + g for g in range(4)] for i in range(N)], 1))
    for bit, pos in _sites(Cn, N, O):
        if bit in (4, 8) and families & bit:
            out.append((L if bit == 4 else 4, [[q] for q in pos], pos[1] - pos[0] if N > 1 else 1))
    return out


def _candidates(Cn, N, O, L, families, d):
    """the definition, restated: (changes the signature, (first, stride, count, value)) of every candidate - every run of a unit to every
    alternative its bytes do not all hold - in the order unit, run, value"""
    out = []
    for alts, steps, stride in _units(Cn, N, O, L, families):
        w = len(steps[0])
        i0 = 1
        while i0 < N:
            tup = [int(d[q]) for q in steps[i0]]
            if min(tup) < 0:
                i0 += 1
                continue
            i1 = i0
            while i1 + 1 < N and [int(d[q]) for q in steps[i1 + 1]] == tup:
                i1 += 1
            for v in range(alts):
                if all(x == v for x in tup):
                    continue
                changes = False
                for k in range(w):
                    b = [int(d[steps[i][k]]) for i in range(N)]
                    nb = list(b)
                    nb[i0:i1 + 1] = [v] * (i1 - i0 + 1)
                    changes = changes or _collapsed(nb) != _collapsed(b)
                out.append((changes, (steps[i0][0], stride, w * (i1 - i0 + 1), v)))
            i0 = i1 + 1
    return out


def _apply(d, mv):
    n = np.array(d, dtype=np.int8)
    for k in range(mv[2]):
        n[mv[0] + k * mv[1]] = mv[3]
    return n


def _jumps(Cn, N, O, L, fam, d):
    return [tuple(int(x) for x in r) for r in P.pool_jumps(Cn, N, O, L, fam, d)]


def test_the_exports_exist(lib):
    hdr = open(os.path.join(ROOT, "include", "miqp_gpu.h")).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in P.wrapper.EXPORTED_SYMBOLS
        assert n + "(" in hdr, n
    assert "IloCplex::populate" in hdr
    assert "miqp_pool_explore_c" in open(os.path.join(ROOT, "include", "miqp_types.h")).read()


def test_the_struct_is_the_librarys(lib):
    assert lib.miqp_gpu_pool_explore_size() == C.sizeof(PoolExploreC) == 40
    assert [n for n, _ in PoolExploreC._fields_] == ["parent", "pass_", "first", "stride", "count", "value", "iterations", "reserved", "objective"]


@pytest.mark.parametrize("dims", DIMS)
def test_the_jumps_are_the_definition(lib, dims):
    """random records with bytes in -1 .. 4 (step 0 too; 4 is the soft alternative of an obstacle with 4 edges), one of them with long runs, every
    families value 1 .. 15: the library's jumps are the candidates of the restatement that change the signature, in its order, cut at
    pool_moves_max(); every returned jump changes pool_signature under that families and every dropped candidate leaves it as it is; no jump writes
    step 0 or an undecided byte, none has the soft value"""
    Cn, N, O = dims
    D = _layout(Cn, N, O)[3]
    rng = np.random.default_rng(8000 + 1000 * Cn + 10 * N + O)
    recs = [rng.integers(-1, 5, size=D).astype(np.int8), np.repeat(rng.integers(-1, 5, size=(D + 2) // 3), 3)[:D].astype(np.int8)]
    for ci in range(Cn * O):   # groups with long tuple runs: five points on one edge for a stretch of steps
        f_obs = _layout(Cn, N, O)[1]
        for i in range(1, N):
            if (i // 3 + ci) % 2:
                recs[1][f_obs + (ci * N + i) * 5:f_obs + (ci * N + i) * 5 + 5] = (i // 3 + ci) % 5
    step0 = {pos[0] for _, pos in _sites(Cn, N, O)}
    cut = dropped = total = 0
    for d in recs:
        for fam in range(1, 16):
            if not fam & 12:
                with pytest.raises(ValueError):
                    P.pool_jumps(Cn, N, O, LINES, fam, d)
                continue
            cand = _candidates(Cn, N, O, LINES, fam, d)
            want = [mv for changes, mv in cand if changes]
            cut += len(want) > P.pool_moves_max()
            dropped += len(cand) - len(want)
            got = P.pool_jumps(Cn, N, O, LINES, fam, d)
            assert got.dtype == np.int32 and got.shape == (min(len(want), P.pool_moves_max()), 4)
            assert [tuple(int(x) for x in r) for r in got] == want[:P.pool_moves_max()], (dims, fam)
            total += len(got)
            sig = P.pool_signature(Cn, N, O, fam, d).tobytes()
            for changes, mv in cand:
                first, stride, count, value = mv
                assert 0 <= value < (LINES if first < _layout(Cn, N, O)[2] else 4)
                for k in range(count):
                    q = first + k * stride
                    assert q < D and q not in step0 and d[q] >= 0, (dims, fam, mv)
                assert (P.pool_signature(Cn, N, O, fam, _apply(d, mv)).tobytes() != sig) == changes, (dims, fam, mv, changes)
    if dims == (2, 20, 4):
        assert cut   # (conditions on the inputs: this shape's records have more jumps than the cap, so the cut is exercised ...
    if N > 2:
        assert total   # ... every shape with a horizon has jumps ...
    if N >= 6:
        assert dropped   # ... and candidates that only move a change point)


def _obstacle_record(N, rows):
    """one car, one obstacle: rows[i] the five point bytes of step i; every other byte undecided"""
    D = _layout(1, N, 1)[3]
    d = np.full(D, -1, dtype=np.int8)
    f_obs = _layout(1, N, 1)[1]
    for i, r in enumerate(rows):
        d[f_obs + i * 5:f_obs + i * 5 + 5] = r
    return d, f_obs


def test_hand_written_records():
    U = [-1] * 5
    # an all-undecided record gives no jump, and a site that is undecided everywhere gives none beside decided ones
    d, f = _obstacle_record(6, [U] * 6)
    assert _jumps(1, 6, 1, 3, 4, d) == []
    d, f = _obstacle_record(4, [U, [0, -1, -1, -1, -1], [0, -1, -1, -1, -1], [0, -1, -1, -1, -1]])
    assert _jumps(1, 4, 1, 3, 4, d) == [(f + 5, 5, 3, 1), (f + 5, 5, 3, 2)]   # no group jump (a point is undecided), point 0 alone: its run to 1 and to 2
    # step 0 decided: it is neither written nor part of a run
    d, f = _obstacle_record(3, [[1] * 5, [1] * 5, [1] * 5])
    got = _jumps(1, 3, 1, 3, 4, d)
    assert got[:2] == [(f + 5, 1, 10, 0), (f + 5, 1, 10, 2)] and len(got) == 2 + 5 * 2 and got[2:4] == [(f + 5, 5, 2, 0), (f + 5, 5, 2, 2)]
    # a run of length 1 between two other runs (steps 1 .. 5: 0 0 2 1 1): the group has the runs [1, 2], [3, 3], [4, 5]; with maximal runs of fully
    # decided bytes every jump replaces or merges an element of the collapsed sequence 0 2 1, so all of them stay
    rows = [U, [0] * 5, [0] * 5, [2] * 5, [1] * 5, [1] * 5]
    d, f = _obstacle_record(6, rows)
    grp = [j for j in _jumps(1, 6, 1, 3, 4, d) if j[1] == 1]
    assert grp == [(f + 5, 1, 10, 1), (f + 5, 1, 10, 2), (f + 15, 1, 5, 0), (f + 15, 1, 5, 1), (f + 20, 1, 10, 0), (f + 20, 1, 10, 2)], grp
    # one point changes its edge a step later than the other four (point 0: 0 0 1 1, the others 0 1 1 1): the group's run [2, 2] lies inside point 0's
    # run of 0 and inside the others' run of 1, so either jump of it only moves a change point of the sites it writes - no jump; [1, 1] and [3, 4] jump
    rows = [U, [0] * 5, [0, 1, 1, 1, 1], [1] * 5, [1] * 5]
    d, f = _obstacle_record(5, rows)
    grp = [j for j in _jumps(1, 5, 1, 2, 4, d) if j[1] == 1]
    assert grp == [(f + 5, 1, 5, 1), (f + 15, 1, 10, 0)], grp
    # a tuple run broken by one undecided point: steps 1 .. 2 and 4 .. 5 are runs of the group, step 3 is none; point 2 alone has the runs [1, 2], [4, 5]
    # with an undecided byte between them, the other points [1, 5]
    rows = [U, [0] * 5, [0] * 5, [0, 0, -1, 0, 0], [0] * 5, [0] * 5]
    d, f = _obstacle_record(6, rows)
    got = _jumps(1, 6, 1, 2, 4, d)
    assert got[:2] == [(f + 5, 1, 10, 1), (f + 20, 1, 10, 1)], got
    assert got[2:] == [(f + 5, 5, 5, 1), (f + 6, 5, 5, 1), (f + 7, 5, 2, 1), (f + 22, 5, 2, 1), (f + 8, 5, 5, 1), (f + 9, 5, 5, 1)], got
    # N = 3, two steps that differ: the group jump of step 1 to the edge of step 2 would merge the two runs - it changes the signature, so it stays
    d, f = _obstacle_record(3, [U, [0] * 5, [1] * 5])
    grp = [j for j in _jumps(1, 3, 1, 2, 4, d) if j[1] == 1]
    assert grp == [(f + 5, 1, 5, 1), (f + 10, 1, 5, 0)], grp
    d, f = _obstacle_record(2, [U, [0] * 5])   # N = 2: one step to write
    assert _jumps(1, 2, 1, 2, 4, d) == [(f + 5, 1, 5, 1)] + [(f + 5 + pt, 5, 1, 1) for pt in range(5)]
    assert _jumps(1, 1, 1, 2, 4, _obstacle_record(1, [[0] * 5])[0]) == []
    # a group already all v: no jump to v; a run that holds the soft alternative is jumped from, never to
    d, f = _obstacle_record(3, [U, [2] * 5, [2] * 5])
    got = _jumps(1, 3, 1, 2, 4, d)
    assert [j for j in got if j[1] == 1] == [(f + 5, 1, 10, 0), (f + 5, 1, 10, 1)] and all(j[3] in (0, 1) for j in got)
    d, f = _obstacle_record(3, [U, [1] * 5, [1] * 5])
    assert [j for j in _jumps(1, 3, 1, 2, 4, d) if j[1] == 1] == [(f + 5, 1, 10, 0)]
    # a car pair: the four group-sites of the pair jump together, alternatives 0 .. 3; the obstacle family alone gives the pair nothing
    D = _layout(2, 3, 0)[3]; f_c2c = _layout(2, 3, 0)[2]
    d = np.full(D, -1, dtype=np.int8); d[f_c2c + 4:f_c2c + 12] = 1
    got = _jumps(2, 3, 0, 0, 8, d)
    assert got[:3] == [(f_c2c + 4, 1, 8, 0), (f_c2c + 4, 1, 8, 2), (f_c2c + 4, 1, 8, 3)] and got[3:6] == [(f_c2c + 4, 4, 2, 0), (f_c2c + 4, 4, 2, 2), (f_c2c + 4, 4, 2, 3)]
    assert len(got) == 3 + 4 * 3 and _jumps(2, 3, 0, 0, 12, d) == got and _jumps(2, 3, 0, 0, 4, d) == []
    # region and environment sites never jump
    d = np.zeros(_layout(1, 4, 0)[3], dtype=np.int8)
    assert _jumps(1, 4, 0, 3, 15, d) == []


def test_error_codes(lib):
    Cn, N, O = 2, 6, 1
    D = _layout(Cn, N, O)[3]
    d = np.random.default_rng(3).integers(0, 4, size=D).astype(np.int8)
    out = np.zeros((512, 4), dtype=np.int32)
    dp, op = d.ctypes.data_as(BP), out.ctypes.data_as(IP)
    n = lib.miqp_gpu_pool_jumps(Cn, N, O, LINES, 12, dp, op, 512)
    assert n > 1
    assert lib.miqp_gpu_pool_jumps(Cn, N, O, LINES, 12, None, op, 512) == -1 and lib.miqp_gpu_pool_jumps(Cn, N, O, LINES, 12, dp, None, 512) == -1
    assert lib.miqp_gpu_pool_jumps(0, N, O, LINES, 12, dp, op, 512) == -1 and lib.miqp_gpu_pool_jumps(Cn, 0, O, LINES, 12, dp, op, 512) == -1
    assert lib.miqp_gpu_pool_jumps(Cn, N, -1, LINES, 12, dp, op, 512) == -1 and lib.miqp_gpu_pool_jumps(Cn, N, O, -1, 12, dp, op, 512) == -1
    for fam in (0, 16, 28, 31, 32, -1, 1, 2, 3):   # outside 1 .. 15, or neither the obstacle nor the car/car family
        assert lib.miqp_gpu_pool_jumps(Cn, N, O, LINES, fam, dp, op, 512) == -2, fam
    assert lib.miqp_gpu_pool_jumps(Cn, N, O, LINES, 12, dp, op, n - 1) == -3 and lib.miqp_gpu_pool_jumps(Cn, N, O, LINES, 12, dp, op, n) == n
    for fam in (0, 3, 16, 31):
        with pytest.raises(ValueError):
            P.pool_jumps(Cn, N, O, LINES, fam, d)
    with pytest.raises(ValueError):
        P.pool_jumps(Cn, N, O, LINES, 12, d[:-1])


def test_explore_answers_before_any_device(lib):
    """the filter and the number of passes are checked first; a handle whose pool is empty returns 0 without touching a device; the pool is as before"""
    w = _loaded()
    assert w.setSolutionPool(8) == 0
    out = (PoolExploreC * 16)()
    assert lib.miqp_solver_pool_explore(None, 4, -1.0, out, 16) == -1 and lib.miqp_solver_pool_explore(w._h, 4, -1.0, None, 16) == -1
    assert lib.miqp_solver_pool_explore(w._h, 4, -1.0, out, -1) == -1 and lib.miqp_solver_pool_explore(w._h, 4, float("nan"), out, 16) == -1
    for fam in (0, 1, 2, 3, 16, 28, 31):
        assert w.setSolutionPoolFilter(fam) == 0
        rc, added = w.exploreSolutionPool()
        assert rc == -2 and added == [], (fam, rc)
        assert w.solutionPoolCount() == 0 and len(w.solutionPoolFound()) == 0
    for fam in (4, 8, 12, 15):
        assert w.setSolutionPoolFilter(fam) == 0
        for passes in (0, -1, 65):
            assert w.exploreSolutionPool(passes)[0] == -2, (fam, passes)
        assert w.exploreSolutionPool() == (0, []) and w.exploreSolutionPool(1, 0.5) == (0, [])   # (no solve yet: the pool is empty, with or without a device)
        assert w.solutionPoolCount() == 0 and w.solutionPoolFoundDecisions(0) is None
    import torch
    if not torch.cuda.is_available():
        assert w.callCplex() != P.OptimizationStatus.SUCCESS and w.exploreSolutionPool() == (0, []) and w.solutionPoolCount() == 0
    fresh = P.CplexWrapper()
    assert lib.miqp_solver_pool_explore(fresh._h, 4, -1.0, out, 16) == -1   # no instance

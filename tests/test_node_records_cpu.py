"""The node records of helpers.py (canonical, relaxed, infeasible) against the CPU oracle alone: what test_node_qp_gpu.py feeds the device
is checked here without one."""
import numpy as np
import pytest

import helpers as H


def _zeros_per_disjunction(r):
    yield from (np.sum(getattr(r, n) == 0, axis=1) for n in H.ENV_FIELDS)
    yield np.sum(r.deltacc == 0, axis=3)
    yield np.sum(r.deltacc_front == 0, axis=3)
    yield np.sum(H._c2c_view(r) == 0, axis=4)


@pytest.mark.parametrize("name", list(H.NODE_SHAPES))
def test_canonical_and_relaxed_records_are_feasible_and_well_posed_for_the_oracle(oracle, name):
    """one 0 per leaf disjunction after canonicalisation; every level keeps the regions and only removes zeros; the oracle returns rc 0 on every
    level, and its own answer moves by less than the node test's bounds between QP_TOL_FINAL and a tolerance 100 times looser (else the QP is
    degenerate and its seed has to be replaced: the list beside NODE_SHAPES)"""
    p, h, dims, rec = H.node_instance(oracle, name)
    assert dims == H.shape_dims(name)
    assert all(z.max(initial=0) <= 1 for z in _zeros_per_disjunction(rec))
    D = H.leaf_disjunctions(rec)
    assert dims[3] != 1 or not any(cls.startswith("env") for cls, key in D)
    levels = H.relax_levels(rec, H.RELAX_SEED[name])
    assert list(levels) == H.level_names(dims)
    objs = {}
    for lname, (r, decided) in levels.items():
        assert np.array_equal(r.active_region, rec.active_region) and np.array_equal(r.region_change_not_allowed_combined, rec.region_change_not_allowed_combined)
        assert len(H.leaf_disjunctions(r)) == decided
        for n in H.ENV_FIELDS + ["deltacc", "deltacc_front", "car2car_collision"]:
            assert np.all((getattr(r, n) == getattr(rec, n)) | (getattr(r, n) == 1)), (lname, n)
        st, res, obj, it = oracle.solve_fixed(h, dims, r)
        st2, res2, obj2, it2 = oracle.solve_fixed(h, dims, r, qp_tol=1e-11)
        assert st == 0 and st2 == 0, (name, lname, st, st2)
        spread = max(np.abs(getattr(res, n) - getattr(res2, n)).max() for n in H.CONT_FIELDS)
        assert abs(obj - obj2) <= 1e-7 * max(1.0, abs(obj)) and spread <= 1e-5, (name, lname, obj - obj2, spread)
        objs[lname] = obj
    assert levels["complete"][1] == len(D)
    if len(levels) > 1:
        assert levels["regions_only"][1] == 0
        assert objs["regions_only"] <= objs["two_thirds"] + 1e-7 and objs["two_thirds"] <= objs["third"] + 1e-7 and objs["third"] <= objs["complete"] + 1e-7   # (nested relaxations)


BIND = 1e-3   # an objective this far above the regions-only one: rows of the level bind (the objectives are 20 to 300, the oracle's own error below 1e-7 of them)


@pytest.mark.parametrize("name", [n for n in H.NODE_SHAPES if len(H.level_names(H.shape_dims(n))) > 1])
def test_the_leaf_rows_of_every_shape_bind(oracle, name):
    """a slack row passes with a wrong right-hand side, so on every shape that has leaf disjunctions the complete record costs the oracle more than
    its regions alone: rows that the levels drop were binding"""
    p, h, dims, rec = H.node_instance(oracle, name)
    levels = H.relax_levels(rec, H.RELAX_SEED[name])
    objs = {l: oracle.solve_fixed(h, dims, levels[l][0])[2] for l in ("complete", "regions_only")}
    assert objs["complete"] > objs["regions_only"] + BIND, objs


@pytest.mark.parametrize("cls,name", [(c, n) for c, names in H.CLASS_BINDS_ON.items() for n in names])
def test_every_row_class_binds_on_its_own_somewhere(oracle, cls, name):
    """environment front points (a second piece narrower than the first), obstacle rear points (on the hexagon: slanted edges, general rows),
    obstacle front points and car/car rows each bind with only that class decided"""
    p, h, dims, rec = H.node_instance(oracle, name)
    levels = H.relax_levels(rec, H.RELAX_SEED[name])
    objs = {l: oracle.solve_fixed(h, dims, levels[l][0])[2] for l in ("only_" + cls, "regions_only")}
    assert objs["only_" + cls] > objs["regions_only"] + BIND, objs


def test_every_row_class_has_a_shape_on_which_it_binds():
    assert set(H.CLASS_BINDS_ON) == {"env_front", "obs_rear", "obs_front", "c2c"} and all(H.CLASS_BINDS_ON.values())


# ---------------------------------------------------------------------------------------------------------------------
# soft levels (helpers.SOFT_CASES): conditions on the reference alone, so that test_node_qp_soft_gpu.py can tell a wrong kernel from a right one
_SOFT_IDS = [H.soft_tag(n, m) for n, m in H.SOFT_CASES]
# The cases whose returned record costs the raw model MORE than the node, and by how much of the node's objective (measured): on cfg4's shape the undecided
# third holds car/car disjunctions whose completed side needs slack, which the raw model prices and the relaxation does not.  Everywhere else - all decided
# levels, and this level on the other five cases - the two objectives are equal to 1e-9.
SOFT_RAW_ABOVE = {("c2n20a", (0, 1, 0, 0), "soft_third_undecided"): 2.437971e-05, ("c2n20a", (1, 0, 0, 0), "soft_third_undecided"): 2.327709e-05,
                  ("c2n20b", (0, 1, 0, 0), "soft_third_undecided"): 1.422437e-02}


@pytest.mark.parametrize("name,mask", H.SOFT_CASES, ids=_SOFT_IDS)
def test_soft_levels_are_feasible_priced_and_well_posed_for_the_oracle(oracle, name, mask):
    """Every soft level differs from the record it starts from at the ignored points alone (all their deltacc entries 1, their slack entries 1) and
    is feasible for the oracle.  The oracle's objective is that of its returned record under the raw big-M statement (raw_eval charges
    WEIGHTS_SLACK_OBSTACLE * s^2 itself) within 1e-9 relative, with no raw row violated - except on soft_third_undecided of cfg4's shape, where the
    undecided car/car disjunctions cost the completed record slack that the relaxation does not pay: there the raw objective lies ABOVE the node's by
    the measured share of SOFT_RAW_ABOVE (2.4e-5 and 2.3e-5 on c2n20a, 1.4e-2 on c2n20b).
    The returned record carries exactly the ignored points in slackvarsObstacle*, and the degeneracy rule of the hard levels holds: the states move
    by less than 1e-5 between QP_TOL_FINAL and a tolerance 100 times looser.  c2n20b's soft_third_undecided broke that rule with the odd steps
    ignored (1.38e-5) and ignores the even steps instead (3.0e-6): helpers.SOFT_EVEN_STEPS."""
    p, h, dims, rec = H.soft_instance(oracle, name, mask)
    assert rec is H.node_instance(oracle, name)[3] and h != H.node_instance(oracle, name)[1]
    assert list(p.obstacle_is_soft) == list(mask) and p.WEIGHTS_SLACK_OBSTACLE == H.SOFT_WEIGHT
    third = H.relax_levels(rec, H.RELAX_SEED[name])["third"][0]
    levels = H.soft_levels(name, rec, mask)
    assert list(levels) == H.SOFT_LEVELS
    for lname, (r, pts) in levels.items():
        assert pts and len(set(pts)) == len(pts) and all(mask[o] == 1 and i >= 1 for c, o, i, pt in pts), (name, lname)
        assert H.ignored_points(r) == pts
        start = H.copy_record(third if lname == "soft_third_undecided" else rec)
        H.mark_ignored(start, pts)
        for n in H.BIN_FIELDS + ["car2car_collision", "slackvarsObstacle", "slackvarsObstacle_front"]:
            assert np.array_equal(getattr(r, n), getattr(start, n)), (name, lname, n)
        for c, o, i, pt in pts:
            assert np.all((r.deltacc[c, o, i] if pt == 0 else r.deltacc_front[c, o, i, :, pt - 1]) == 1)
        st, res, obj, it = oracle.solve_fixed(h, dims, r)
        st2, res2, obj2, it2 = oracle.solve_fixed(h, dims, r, qp_tol=1e-11)
        assert st == 0 and st2 == 0, (name, lname, st, st2)
        assert H.ignored_points(res) == pts, (name, lname)
        v, robj, worst = oracle.raw_eval(h, res)
        assert v < 1e-9, (name, lname, worst, v)
        if (name, mask, lname) in SOFT_RAW_ABOVE:
            gap = SOFT_RAW_ABOVE[(name, mask, lname)]
            assert abs((robj - obj) / obj - gap) <= 1e-3 * gap, (name, lname, robj, obj, (robj - obj) / obj)
        else:
            assert abs(robj - obj) <= 1e-9 * max(1.0, abs(obj)), (name, lname, robj, obj)
        spread = max(np.abs(getattr(res, n) - getattr(res2, n)).max() for n in H.CONT_FIELDS)
        assert abs(obj - obj2) <= 1e-7 * max(1.0, abs(obj)) and spread <= 1e-5, (name, lname, obj - obj2, spread)
    assert len(levels["soft_all"][1]) == dims[0] * (dims[1] - 1) * 5
    assert len(levels["soft_rear"][1]) + len(levels["soft_front"][1]) == len(levels["soft_all"][1])


# (shape, mask): the levels on which the rows of the ignored points BIND - drop, the hard complete objective minus (soft objective - SOFT_WEIGHT *
# points), exceeds BIND - with the drop measured.  On c2n6e2pent, c2n20b and c2n20a with mask [1, 0, 0, 0] the soft obstacle's rows are slack (drop
# 0 to 1e-10): those cases pin the price and the decode of the byte alone.
SOFT_BINDS = {("c1n2r32o", (1,)): {"soft_all": 1.146, "soft_front": 1.146}, ("c1n6r16hex", (1,)): {"soft_all": 5.946, "soft_front": 5.559, "soft_odd_steps": 5.946},
              ("c2n20a", (0, 1, 0, 0)): {"soft_all": 26.22, "soft_front": 25.76, "soft_odd_steps": 15.72}, ("c1n21o", (1,)): {"soft_all": 25.65, "soft_front": 25.07},
              ("c3n6o", (1,)): {"soft_all": 0.3156, "soft_front": 0.3156, "soft_odd_steps": 0.3156}}


@pytest.mark.parametrize("name,mask", list(SOFT_BINDS), ids=[H.soft_tag(n, m) for n, m in SOFT_BINDS])
def test_the_ignored_rows_of_a_soft_obstacle_bind(oracle, name, mask):
    """a kernel that kept the row of an ignored point would pass where that row is slack anyway: on these levels dropping the rows lowers the
    oracle's objective, net of the price, by more than BIND"""
    p, h, dims, rec = H.soft_instance(oracle, name, mask)
    hard = oracle.solve_fixed(H.node_instance(oracle, name)[1], dims, rec)[2]
    levels = H.soft_levels(name, rec, mask)
    for lname, measured in SOFT_BINDS[(name, mask)].items():
        r, pts = levels[lname]
        drop = hard - (oracle.solve_fixed(h, dims, r)[2] - H.SOFT_WEIGHT * len(pts))
        assert drop > BIND and abs(drop - measured) <= 1e-2 * measured, (name, lname, drop, measured)


def test_the_soft_cases_reach_every_kind_of_shape():
    """N = 2, L = 6 and 5 (byte L is not 4), two cars on the on-chip blocks, a soft obstacle that is not obstacle 0 beside hard ones, more than 20 steps,
    three cars; and the rows bind on a one-car on-chip shape, on cfg4's shape, beyond the on-chip kernels and on the wide kernel"""
    dims = [H.shape_dims(n) for n, m in H.SOFT_CASES]
    assert any(d[1] == 2 for d in dims) and {5, 6} <= {d[5] for d in dims} and any(d[0] == 3 for d in dims) and any(d[1] > 20 for d in dims)
    assert any(len(m) > 1 and m[0] == 0 for n, m in H.SOFT_CASES) and any(len(m) > 1 and m[0] == 1 for n, m in H.SOFT_CASES)
    assert all(k in H.SOFT_CASES for k in SOFT_BINDS) and {"c1n6r16hex", "c2n20a", "c1n21o", "c3n6o"} <= {n for n, m in SOFT_BINDS}


@pytest.mark.parametrize("k", range(len(H.INFEASIBLE_NODES)))
def test_infeasible_records_are_infeasible_for_the_oracle(oracle, k):
    name, cls, key, alt = H.INFEASIBLE_NODES[k]
    p, h, dims, rec = H.node_instance(oracle, name)
    assert key[2] == 1   # step 1: the initial state pins the position
    bad = H.infeasible_record(rec, cls, key, alt)
    assert len(H.leaf_disjunctions(bad)) == len(H.leaf_disjunctions(rec))
    st, res, obj, it = oracle.solve_fixed(h, dims, bad)
    assert st == 1, (name, cls, key, alt, st)
    st, res, obj, it = oracle.solve_fixed(h, dims, rec)
    assert st == 0


def test_every_shape_with_infeasible_records_has_at_least_two():
    names = [n for n, _, _, _ in H.INFEASIBLE_NODES]
    assert set(names) == {"c1n6r32o", "mini", "c2n20a"} and all(names.count(n) >= 2 for n in set(names))

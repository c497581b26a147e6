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

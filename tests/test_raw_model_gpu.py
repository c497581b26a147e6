"""`worst_row` of a certificate names a row of the exported .lp: the row c<worst_row+1> of miqp_solver_export_lp, evaluated in
Python on the certified record, is violated by the certificate's max_violation.  One perturbed member per row family."""
import numpy as np
import pytest

import planner_miqp_amd as P
from helpers import copy_record, lp_case_params, lp_row_violation, parse_lp_rows, record_values

pytestmark = pytest.mark.gpu


def perturbations(p, rec):
    """[(family, use_real_slack, change)] for a solved record: one member per family that the shape has"""
    C_, N, R, E, O, L = rec.dims
    i = 3

    def pos(r): r.pos_x[0, i] += 0.5

    def vel(r): r.vel_x[0, i] = p.max_vel_x_y + 1.0

    def region(r):
        j = int(np.argmax(r.active_region[0, i])); r.active_region[0, i, :] = 0; r.active_region[0, i, (j + R // 2) % R] = 1

    def env(r): r.notWithinEnvironmentRear[0, 0, i] = 1 - r.notWithinEnvironmentRear[0, 0, i]

    def obstacle(r): r.deltacc[0, 0, i, r.deltacc[0, 0, i] == 0] = 1          # the side the car is on: no side is left

    def car(r): r.car2car_collision[0, 0, i, :4][r.car2car_collision[0, 0, i, :4] == 0] = 1

    out = [(2, True, pos), (3, True, vel), (4, True, region), (6, True, env)]
    if O > 0:
        out.append((7, True, obstacle))
    if C_ > 1:
        out.append((8, False, car))
    return out


@pytest.mark.parametrize("case", ["mini:0", "mini1soft:0", "mini3:0"])
def test_worst_row_is_the_row_of_the_exported_file(tmp_path, case):
    p = lp_case_params(case)
    p.relative_mip_gap_tolerance = 1e-4
    w = P.CplexWrapper()
    w.resetParameters(p)
    assert w.callCplex() == P.OptimizationStatus.SUCCESS
    path = str(tmp_path / "m.lp")
    assert P.load_library().miqp_solver_export_lp(w._h, path.encode()) == 0
    rows = parse_lp_rows(open(path).read())
    rec = w.getRawResults()
    base = w.certify(rec)
    assert base.rows == len(rows) and base.max_violation < 1e-5
    todo = perturbations(p, rec)
    assert [f for f, _, _ in todo] == [2, 3, 4, 6] + ([7] if rec.dims[4] else []) + ([8] if rec.dims[0] > 1 else [])
    for family, real, change in todo:
        r2 = copy_record(rec)
        change(r2)
        cert = w.certify(r2, use_real_slack=real)
        v = cert.max_violation
        print(case, "A%d" % family, "max_violation", v, "family", cert.worst_family, "row", cert.worst_row)
        assert v > 1e-3 and cert.family_violation[family - 1] > 1e-3, (family, cert)
        values = record_values(r2, real)
        tol = 1e-9 * max(1.0, v)
        assert abs(lp_row_violation(rows[cert.worst_row], values) - v) <= tol, (family, cert, rows[cert.worst_row])
        assert max(lp_row_violation(row, values) for row in rows) <= v + tol      # and no row of the file is violated by more

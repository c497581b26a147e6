"""Certificate of delivered records against the raw big-M model, the part that needs no GPU: ABI, refusals, and the .lp
writer that shares its row order with the certificate."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest

import planner_miqp_amd as P
from helpers import dat_path, k3_results
from planner_miqp_amd.ctypes_types import CertificateC, RawResults

# sha256 of miqp_solver_export_lp for cplexmodel_testcase.dat, recorded before the certificate was added
LP_SHA256_TESTCASE = "aaebaa90f5594036b9561c2de9d777b8026818f8f3d4b34d8a81a144e63c3043"


@pytest.fixture(scope="module")
def lib():
    P.build_library()
    return P.load_library()


def _wrapper(name="cplexmodel_testcase.dat"):
    w = P.CplexWrapper(parameterSource=P.ParameterSource.DATFILE)
    w.setParameterDatFileAbsolute(dat_path(name))
    assert w._push_inputs() == 0
    return w


def test_symbols_and_struct_size(lib):
    for n in ("miqp_solver_certify", "miqp_solver_certify_batch", "miqp_gpu_certificate_size", "miqp_gpu_certify_last_timing"):
        assert hasattr(lib, n), n
    assert C.sizeof(CertificateC) == lib.miqp_gpu_certificate_size() == 104
    assert callable(P.certify_batch) and callable(P.CplexWrapper.certify) and P.Certificate is not None


def test_handle_without_a_solution_reports_status_1(lib):
    w = _wrapper()
    out = CertificateC()
    assert lib.miqp_solver_certify(w._h, None, C.byref(out)) == 0
    assert out.status == 1 and out.rows == -1 and out.worst_row == -1 and out.worst_family == -1
    assert math.isnan(out.max_violation) and math.isnan(out.objective) and math.isnan(out.max_int_infeas)
    assert all(math.isnan(v) for v in out.family_violation)
    c = w.certify()
    assert c.status == 1 and "no solution" in repr(c)
    many = P.certify_batch([w, _wrapper()])
    assert [m.status for m in many] == [1, 1]


def test_candidate_of_another_shape_is_refused(lib):
    w = _wrapper()
    out = CertificateC()
    for dims in ((1, 19, 32, 1, 1, 4), (2, 20, 32, 1, 1, 4), (1, 20, 16, 1, 1, 4), (1, 20, 32, 2, 1, 4), (1, 20, 32, 1, 2, 4)):
        r = RawResults(*dims)
        rc = r.to_c()
        assert lib.miqp_solver_certify(w._h, C.byref(rc), C.byref(out)) == -3, dims
    r, _ = k3_results()
    rc = r.to_c()
    rc.pos_x = None
    assert lib.miqp_solver_certify(w._h, C.byref(rc), C.byref(out)) == -2
    assert lib.miqp_solver_certify(None, None, C.byref(out)) < 0 and lib.miqp_solver_certify(w._h, None, None) < 0


def test_no_host_evaluation_without_a_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    w = _wrapper()
    r, _ = k3_results()
    rc = r.to_c()
    out = CertificateC()
    out.max_violation = -7.0; out.rows = -7
    assert lib.miqp_solver_certify(w._h, C.byref(rc), C.byref(out)) < 0
    assert "no HIP device" in w.lastError() and "no host evaluation" in w.lastError()
    assert out.max_violation == -7.0 and out.rows == -7          # nothing was evaluated
    with pytest.raises(RuntimeError, match="no HIP device"):
        w.certify(r)


def test_lp_export_is_byte_identical(lib, tmp_path):
    w = _wrapper()
    path = str(tmp_path / "t.lp")
    assert lib.miqp_solver_export_lp(w._h, path.encode()) == 0
    data = open(path, "rb").read()
    assert hashlib.sha256(data).hexdigest() == LP_SHA256_TESTCASE
    assert data.count(b"\n c") == w.rawSizes()["rows"] == 12361   # rows c1..c12361: worst_row + 1 names a row of this file


def test_certificate_class_mirrors_the_struct():
    c = CertificateC()
    c.max_violation = 0.5; c.objective = 2.0; c.family_violation[1] = 0.5; c.worst_family = 2; c.worst_row = 7; c.rows = 10
    k = P.Certificate(c)
    assert k.max_violation == 0.5 and k.worst_family == 2 and k.worst_row == 7 and k.rows == 10 and k.status == 0
    assert isinstance(k.family_violation, np.ndarray) and k.family_violation.shape == (8,) and k.family_violation[1] == 0.5
    assert "A2 dynamics" in repr(k) and len(k.raw) == C.sizeof(CertificateC)

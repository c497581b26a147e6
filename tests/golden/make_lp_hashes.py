"""Regenerates tests/golden/lp_sha256.json: sha256 and number of row lines (` c<k>:`) of miqp_solver_export_lp for helpers.LP_CASES.

Recorded from the build BEFORE the .lp writer and the certificate kernel were moved onto one row walker (raw_model.hpp);
tests/test_raw_model_cpu.py holds every later build to these files byte for byte.  Run it only on a commit whose export
is known to be right: it pins whatever the library writes.
"""
import hashlib
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

import planner_miqp_amd as P  # noqa: E402
from helpers import LP_CASES, lp_case_wrapper  # noqa: E402


def main():
    P.build_library()
    lib = P.load_library()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for case in LP_CASES:
            w = lp_case_wrapper(case)
            path = os.path.join(d, "m.lp")
            assert lib.miqp_solver_export_lp(w._h, path.encode()) == 0, case
            data = open(path, "rb").read()
            out[case] = dict(sha256=hashlib.sha256(data).hexdigest(), rows=len(re.findall(rb"^ c\d+:", data, re.M)))
            print(case, out[case])
    json.dump(out, open(os.path.join(HERE, "lp_sha256.json"), "w"), indent=1)


if __name__ == "__main__":
    main()

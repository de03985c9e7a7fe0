"""Writes tests/golden/inter_residual.npz: small pictures (source, prediction, CU map) and every output that the compiled reference's
own kvz_quantize_residual, kvz_pixels_calc_ssd and kvz_coeff_abs_sum compose for them over the transform tree
(tests/inter_residual_cases.py).  Needs the compiled reference (oracle/_ref).  Refuses to write a fixture that does not contain
every TU size with both flag values and the CU kinds listed in inter_residual_cases.coverage."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import inter_residual_cases as RC  # noqa: E402
import ref_lib as R  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    d, missing = RC.build_fixture(R)
    assert not missing, "the fixture lacks: " + ", ".join(missing)
    out = os.path.join(HERE, "golden", "inter_residual.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")

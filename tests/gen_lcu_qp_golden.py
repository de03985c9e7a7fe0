"""Writes tests/golden/lcu_qp.npz: small pictures (source, prediction planes, CU map, modes, a QP per LCU) and every output that the
compiled reference's own functions compose for the chain inter residual -> intra reconstruction -> QP map with the QP of each TU's LCU
(tests/lcu_qp_cases.py).  Needs the compiled reference (oracle/_ref).  Refuses to write a fixture that does not contain what
lcu_qp_cases.coverage lists."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import lcu_qp_cases as QC  # noqa: E402
import ref_lib as R  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    d, missing = QC.build_fixture(R)
    assert not missing, "the fixture lacks: " + ", ".join(missing)
    out = os.path.join(HERE, "golden", "lcu_qp.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")

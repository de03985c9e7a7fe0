"""Writes tests/golden/intra_recon.npz: small pictures (source, entry planes, CU map, modes) and every output that the compiled reference's
own kvz_intra_build_reference, kvz_intra_predict and kvz_quantize_residual compose for them in coding order
(tests/intra_recon_cases.py).  Needs the compiled reference (oracle/_ref).  Refuses to write a fixture that does not contain
what intra_recon_cases.coverage lists."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import intra_recon_cases as RC  # noqa: E402
import ref_lib as R  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    d, missing = RC.build_fixture(R)
    assert not missing, "the fixture lacks: " + ", ".join(missing)
    out = os.path.join(HERE, "golden", "intra_recon.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")

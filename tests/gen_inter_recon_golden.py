"""Writes tests/golden/inter_recon.npz: small pictures (planes, CU maps, PU lists) and the Y / U / V prediction that the compiled
reference's own functions compose for them (tests/inter_recon_cases.py).  Needs the compiled reference (oracle/_ref)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import inter_recon_cases as IC  # noqa: E402
import ref_lib as R  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    out = os.path.join(HERE, "golden", "inter_recon.npz")
    np.savez_compressed(out, **IC.build_fixture(R))
    print(out, os.path.getsize(out), "bytes")

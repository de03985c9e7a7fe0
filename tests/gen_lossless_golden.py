"""Writes tests/golden/lossless.npz: four small pictures (source and prediction planes, CU map, modes) and what
kvz_hip_inter_residual_frame_lossless and then kvz_hip_intra_recon_frame_lossless leave over poisoned outputs, the intra stage with
implicit_rdpcm 0 and 1 (tests/lossless_cases.py).  Every reference array and every prediction comes from the compiled reference's own
kvz_intra_build_reference and kvz_intra_predict.  Needs the compiled reference (oracle/_ref).  Refuses to write a fixture that does not
contain what lossless_cases.coverage lists."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import lossless_cases as LC  # noqa: E402
import ref_lib as R  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    d, missing = LC.build_fixture(R)
    assert not missing, "the fixture lacks: " + ", ".join(missing)
    out = os.path.join(HERE, "golden", "lossless.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")

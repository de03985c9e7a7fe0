"""Writes tests/golden/sao_frame.npz: small pictures (source and deblocked planes, per-LCU SAO records) and what the compiled
reference's own calc_sao_edge_dir and sao_reconstruct_color (with oracle_lib's calc_sao_bands, which the reference's harness does not
export) compose for them per LCU (tests/sao_frame_cases.py): statistics, candidates and the destination planes.  Needs the compiled
reference (oracle/_ref).  Refuses to write a fixture that lacks what sao_frame_cases.coverage lists."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_lib as R  # noqa: E402
import sao_frame_cases as SC  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    d, missing = SC.build_fixture(R)
    assert not missing, "the fixture lacks: " + ", ".join(missing)
    out = os.path.join(HERE, "golden", "sao_frame.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")

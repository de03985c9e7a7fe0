"""Writes tests/golden/trskip.npz: four small pictures (source, prediction planes, CU map, modes, QPs, bit costs) and what
kvz_hip_inter_residual_frame_ts and then kvz_hip_intra_recon_frame_ts leave, the tr_skip map included (tests/trskip_cases.py); for
`mixed` also the chain up to deblocking.  Every trial comes from the compiled reference's own kvz_quantize_residual, `mixed` through
its default scaling lists.  Needs the compiled reference (oracle/_ref).  Refuses to write a fixture that does not contain what
trskip_cases.coverage lists."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_lib as R  # noqa: E402
import trskip_cases as T  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    d, missing = T.build_fixture(R)
    assert not missing, "the fixture lacks: " + ", ".join(missing)
    out = os.path.join(HERE, "golden", "trskip.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")

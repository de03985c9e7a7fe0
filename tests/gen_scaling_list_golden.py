"""Writes tests/golden/scaling_list.npz: the processed default scaling lists as recorded from the compiled reference (packed as
kvz_hip_scaling_tables lays them out), a custom set of lists, three small pictures (source, prediction planes, CU map, modes, QPs) and,
for both list sets, what kvz_hip_inter_residual_frame_sl and then kvz_hip_intra_recon_frame_sl leave (tests/scaling_list_cases.py);
for `ragged` with the custom lists also the chain up to deblocking.  The default-list pictures come from the compiled reference's own
scaling-list path, the custom-list ones from the oracle's table path with tables from the restated list processing.  Needs the compiled
reference (oracle/_ref).  Refuses to write a fixture that does not contain what scaling_list_cases.coverage lists."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_lib as R  # noqa: E402
import scaling_list_cases as SL  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    d, missing = SL.build_fixture(R)
    assert not missing, "the fixture lacks: " + ", ".join(missing)
    out = os.path.join(HERE, "golden", "scaling_list.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")

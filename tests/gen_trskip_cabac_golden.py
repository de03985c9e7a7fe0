"""Writes tests/golden/trskip_cabac.npz: what kvz_hip_inter_residual_frame_ts_cabac and then kvz_hip_intra_recon_frame_ts_cabac leave on
the four pictures of tests/golden/trskip.npz (tests/trskip_cabac_cases.py): every trial from the compiled reference's own
kvz_quantize_residual, every CABAC price from its own counting coder, per-LCU sets and a fast_limit per picture.  Needs the compiled
reference (oracle/_ref).  Refuses to write unless, in every picture, both winners occur among the inter TUs and among the intra TUs it
has, and at least 20 TUs are decided differently under CABAC pricing than under the estimate."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_lib as R  # noqa: E402
import trskip_cabac_cases as K  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    d, why = K.build_fixture(R)
    assert not why, "the fixture cannot tell the entries apart: " + why
    out = os.path.join(HERE, "golden", "trskip_cabac.npz")
    np.savez_compressed(out, **d)
    for pic in K.T.FIXTURE_PICTURES:
        dec = d[pic[0] + "_decided"]
        print("%-6s %4d TUs, %3d skipped, %3d decided differently, %3d priced with CABAC" % (pic[0], len(dec), dec[:, 3].sum(), (dec[:, 3] != dec[:, 4]).sum(),
                                                                                            dec[:, 5].sum()))
    print(out, os.path.getsize(out), "bytes")

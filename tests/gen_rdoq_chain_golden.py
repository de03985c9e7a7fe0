"""Writes tests/golden/rdoq_chain.npz: what kvz_hip_inter_residual_frame_rdoq and then kvz_hip_intra_recon_frame_rdoq leave on the three
pictures of tests/golden/lcu_qp.npz (tests/rdoq_chain_cases.py): every TU from the compiled reference's own kvz_quantize_residual under
cfg.rdoq_enable, which calls kvz_rdoq itself.  Expected outputs only.  Needs the compiled reference (oracle/_ref).  Refuses to write
unless the conditions of rdoq_chain_cases.conditions hold: per picture and stage at least 20 TUs whose levels differ from the plain
quantiser's, one of every width and plane; in `ragged` at least 5 TUs changed by sign hiding and 5 by the set index; in `mono` every 4x4
TU equal to the plain composition and at least 5 larger ones not; tr_depth 0 and above 0 in luma and chroma; a tile grid that matters."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_quant_rdoq as Q  # noqa: E402
import rdoq_chain_cases as K  # noqa: E402

INPUTS = os.path.join(HERE, "golden", "lcu_qp.npz")
OUT = os.path.join(HERE, "golden", "rdoq_chain.npz")


def build():
    assert Q.available(), "the fixture is written from the compiled reference only"
    return K.build_fixture(np.load(INPUTS, allow_pickle=False))


if __name__ == "__main__":
    d, missing = build()
    assert not missing, "the fixture cannot tell the entries apart:\n  " + "\n  ".join(missing)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")

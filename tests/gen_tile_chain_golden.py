"""Writes tests/golden/tile_chain.npz: three small tiled pictures (source, prediction planes, CU map, modes, a QP per LCU, SAO records,
the tile boundaries) and what the compiled reference's own functions, run on every tile as a picture of its own, leave after each stage
of the chain inter residual -> intra reconstruction -> QP map (tiles and LCU rows of tiles as chains) -> deblocking with per_cu_qp = 1 ->
SAO (tests/tile_chain_cases.py).  Needs the compiled reference (oracle/_ref).  Refuses to write a fixture that does not contain what
tile_chain_cases.coverage lists."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_lib as R  # noqa: E402
import tile_chain_cases as TC  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    d, missing = TC.build_fixture(R)
    assert not missing, "the fixture lacks: " + ", ".join(missing)
    out = os.path.join(HERE, "golden", "tile_chain.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")

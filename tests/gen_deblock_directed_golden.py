"""Writes tests/golden/deblock_directed.npz: the directed deblocking pictures (tests/deblock_directed_cases.py) -- planes, CU map,
parameters and tile grid -- and what the compiled reference's kvz_filter_deblock_lcu makes of them, tile by tile for the tiled
picture.  Needs the compiled reference (oracle/_ref).  Refuses to write a fixture whose pictures miss a class of the model's census,
let a mutant of the model through, or on which the model and the reference disagree."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import deblock_directed_cases as DC  # noqa: E402
import deblock_model as M  # noqa: E402
import ref_lib as R  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    DC.assert_coverage(DC.coverage(DC.cases()))
    for c in DC.cases():
        assert DC.first_difference(DC.modelled(c["name"])[0], DC.expected(c, R)) is None, c["name"]
    for mutant in M.MUTANTS:
        for suffix in ("", "^T"):
            assert any(DC.first_difference(DC.modelled(c["name"], mutant)[0], DC.modelled(c["name"])[0])
                       for c in DC.cases() if c["name"].endswith("^T") == bool(suffix)), (mutant, suffix)
    out = os.path.join(HERE, "golden", "deblock_directed.npz")
    np.savez_compressed(out, **DC.build_fixture(R))
    print(out, os.path.getsize(out), "bytes")

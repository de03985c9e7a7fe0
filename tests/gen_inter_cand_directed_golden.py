"""Writes tests/golden/inter_cand_directed.npz: the directed CU maps of the candidate derivation (tests/inter_cand_directed_cases.py) --
parameters, the three maps and the PU list of every case -- and what the compiled reference's kvz_inter_get_merge_cand /
kvz_inter_get_mv_cand make of them (ref_lib.inter_candidates).  Needs the compiled reference (oracle/_ref).  Refuses to write a fixture
whose cases miss a class of the model's census, let a mutant of the model through, or on which the model and the reference disagree."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import inter_cand_directed_cases as DC  # noqa: E402
import inter_cand_model as M  # noqa: E402
import ref_lib as R  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    DC.assert_coverage(DC.coverage(DC.cases()))
    for c in DC.cases():
        assert DC.first_difference(DC.modelled(c[0])[:2], R.inter_candidates(*c[1:])) is None, c[0]
    for mutant in M.MUTANTS:
        assert any(DC.first_difference(DC.modelled(c[0], mutant)[:2], DC.modelled(c[0])[:2]) for c in DC.cases()), mutant
    out = os.path.join(HERE, "golden", "inter_cand_directed.npz")
    np.savez_compressed(out, **DC.build_fixture(R))
    print(out, os.path.getsize(out), "bytes")

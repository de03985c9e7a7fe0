"""Writes tests/golden/me_search_directed.npz: the directed cases of the motion search (tests/me_search_directed_cases.py) -- parameters, the
two planes, the PU list, the CABAC snapshots and the costs to beat of every case -- and what the compiled reference's search makes of them
(ref_lib.search_pu_batch: ref_me_search_pu of oracle/ref_me_harness.c).  Needs the compiled reference (oracle/_ref).  Refuses to write a
fixture whose cases miss a class of the model's census, let a mutant of the model through, or on which the model and the reference disagree."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import me_search_directed_cases as DC  # noqa: E402
import me_search_model as M  # noqa: E402
import ref_lib as R  # noqa: E402

if __name__ == "__main__":
    assert R.available(), "the fixture is written from the compiled reference only"
    DC.assert_coverage(DC.coverage(DC.cases()))
    for c in DC.cases():
        d = DC.first_difference(DC.modelled(c[0])[0], R.search_pu_batch(c[2], c[3], c[4], c[1], cabac=c[5], cost_to_beat=c[6]))
        assert d is None, "%s: the model and the reference differ: %s" % (c[0], d)
    for mutant in M.MUTANTS:
        assert DC.killers(mutant, first_only=True), "the mutant %s (%s) changes no case" % (mutant, M.MUTANTS[mutant])
    out = os.path.join(HERE, "golden", "me_search_directed.npz")
    np.savez_compressed(out, **DC.build_fixture(R))
    print(out, os.path.getsize(out), "bytes")

"""CPU: tests/golden/trskip_cabac.npz holds what its generator demands -- in every picture both winners among the inter and the intra TUs it
has, at least 20 TUs decided differently under CABAC pricing than under the estimate, a picture whose QPs straddle the limit, a picture
without lcu_ctx, a set index beyond the table -- and, where the reference is built, the composition still gives a picture's outputs."""
import os

import numpy as np
import pytest

import ref_lib as R
import trskip_cabac_cases as K
import trskip_cases as T

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "trskip_cabac.npz")


def test_fixture_can_tell_the_pricing_rules_apart():
    z = np.load(GOLDEN, allow_pickle=False)
    assert os.path.getsize(GOLDEN) < 400 * 1000
    for pic in T.FIXTURE_PICTURES:
        name = pic[0]
        dec = z[name + "_decided"]                              # x, y, intra, skip, skip under the estimate, priced with CABAC
        for intra in (0, 1):
            mine = dec[dec[:, 2] == intra]
            assert len(mine) == 0 or set(mine[:, 3].tolist()) == {0, 1}, (name, intra)
        assert (dec[:, 3] != dec[:, 4]).sum() >= K.MIN_DIFFERENT, name
    case = T.fixture_case(T.FIXTURE_PICTURES[2])
    assert case["name"] == "mixed" and min(case["lcu_qp"]) < K.PRICING["mixed"][0] <= max(case["lcu_qp"])
    assert K.lcu_ctx_of(T.fixture_case(T.FIXTURE_PICTURES[0])) is None and max(K.lcu_ctx_of(case)) >= K.N_SETS
    assert len(set(K.lcu_ctx_of(case).tolist())) == len(case["lcu_qp"])
    ranges, dumps = K.context_sets()
    assert (z["ranges"] == ranges).all() and (z["dumps"] == dumps).all() and dumps.max() <= 125


@pytest.mark.skipif(not R.available(), reason="compiled reference not built")
def test_fixture_regenerates_from_the_compiled_reference():
    z = np.load(GOLDEN, allow_pickle=False)
    case = T.fixture_case(T.FIXTURE_PICTURES[3])                 # mono: the smallest
    mid, full = K.compose(case, R)
    assert K.coverage("mono", mid, full) is None
    T.assert_outputs_equal(full, T.load_want(z, "mono", "full", 0), "mono", 0)
    # the model prices as the reference does
    mid2, full2 = K.compose(case, R, use_reference=False)
    T.assert_outputs_equal(full2, full, "mono, priced by the model", 0)

"""CPU: the composed reference of the transform-skip entries (tests/trskip_cases.py) -- the committed fixture against a fresh
composition, from the compiled reference where it was built and from the oracle otherwise; the restated decision on known answers;
what the fixture must contain."""
import os

import numpy as np
import pytest

import oracle_lib as O
import ref_lib as R
import scaling_list_cases as SL
import trskip_cases as T

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "trskip.npz")
LISTS = os.path.join(HERE, "golden", "scaling_list.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def default_tables():
    """the processed default lists as recorded from the reference, for the oracle's table path"""
    z = np.load(LISTS, allow_pickle=False)
    return SL.undense(z["default_quant"], z["default_dequant"])


@pytest.fixture(scope="module")
def fresh(default_tables):
    """the fixture and its coverage, composed once"""
    if R.available():
        return T.build_fixture(R)
    return T.build_fixture(O, default_tables)


def test_fixture_regenerates(golden, fresh):
    """from the compiled reference's own kvz_quantize_residual where oracle/_ref is built, else from the oracle"""
    assert sorted(golden.files) == sorted(fresh[0])
    for k in golden.files:
        np.testing.assert_array_equal(golden[k], fresh[0][k], err_msg=k)


@pytest.mark.skipif(not R.available(), reason="compiled reference not built")
def test_oracle_and_reference_compose_the_same_fixture(golden, default_tables):
    d, _ = T.build_fixture(O, default_tables, probe=False)
    for k in golden.files:
        np.testing.assert_array_equal(golden[k], d[k], err_msg=k)


def test_fixture_is_small_numeric_and_covers_every_branch(golden, fresh):
    assert os.path.getsize(GOLDEN) < 400 * 1000
    assert all(golden[k].dtype.kind in "ui" for k in golden.files)
    assert fresh[1] == [], "coverage"
    pics = {p[0]: p for p in T.FIXTURE_PICTURES}
    assert pics["inter"][1:5] == (72, 72, 1, 1) and pics["intra"][1:5] == (72, 72, 1, 1) and pics["mono"][1:4] == (72, 72, 0)
    assert pics["mixed"][1:4] == (136, 72, 1) and len(pics["mixed"][9]) == 6 and pics["mixed"][10] == ((0, 1, 3), (0, 1, 2)) and pics["mixed"][11]
    assert "mono_src_u" not in golden.files and golden["mixed_bit_cost"].shape == (6,) and len(set(golden["mixed_bit_cost"].tolist())) == 6
    assert golden["inter_bit_cost"].tolist() == [T.lambda_bit_cost(27)] == [18]
    # the three scan orders among the intra picture's 4x4 luma TUs
    case = T.load_case(golden, pics["intra"])
    scans = {t[7] for t in T.XC.walk_tus(case["cus"], case["modes"], 72, 72, 1) if t[0] == 0 and t[3] == 4}
    assert scans == {0, 1, 2}
    # tr_skip is written under the 4x4 luma TUs of the entry's CUs and nowhere else, and both values occur
    for name, pic in pics.items():
        case = T.load_case(golden, pic)
        four = (case["cus"]["tr_depth"] == 4) & (case["cus"]["depth"] == 3)
        for stage, types in (("mid", (T.IC.CU_INTER,)), ("full", (T.IC.CU_INTER, T.IC.CU_INTRA))):
            s = golden["%s_%s_tr_skip" % (name, stage)]
            mine = four & np.isin(case["cus"]["type"], types)
            assert (s[~mine] == T.POISON_SKIP).all() and (s[mine] <= 1).all(), (name, stage)
        assert {0, 1} <= set(golden[name + "_full_tr_skip"].reshape(-1).tolist())
    # and transform skip matters: the flat pictures differ from the composition without it
    case = T.load_case(golden, pics["mono"])
    plain = T.QC.compose_inter(case["src"], case["pred"], case["cus"], case["lcu_qp"], 0, 0, 0, B=O, init=T.QC.zero_outputs(72, 72, 0))
    assert not np.array_equal(plain["coeff"][0], golden["mono_mid_coeff_y"])


def test_coverage_notices_what_is_missing():
    """the check is not vacuous: in a picture of inter CUs whose source is its prediction every TU is a tie, and the rest is missing"""
    case = T.fixture_case(T.FIXTURE_PICTURES[3])
    case["cus"]["type"], case["cus"]["mv_dir"], case["src"] = T.IC.CU_INTER, 1, case["pred"]
    mid, full = T.compose(case, O, probe=T.probe_costs())
    assert len(mid["log"]) > 200 and not full["log"]
    missing = T.coverage({"mono": mid["log"]}, False)
    assert missing == ["mono: the skipped trial is kept in 0 of %d TUs" % len(mid["log"]), "a skipped winner with coefficients",
                       "a TU whose two trials disagree about has_coeffs",
                       "an intra TU whose right or lower neighbour's prediction changes because skip won",
                       "a TU whose decision flips between two bit costs of the fixture"]
    assert len(T.coverage({"none": []}, False)) == 7


def test_decision_known_answers():
    """by hand: qp 27 -> 27 * 0.044407704 + 0.557323653 = 1.756331661; a sum of 10 costs (uint32)(17.56.. + 0.5) = 18, 40 cost 70, 3 cost 5:
    0 + 70 * 7 = 490 <= 500 + 5 * 7 = 535, and 560 > 540"""
    assert T.coeff_cost(10, 27) == 18 and T.coeff_cost(0, 51) == 0 and T.coeff_cost(1, 0) == 1
    assert T.decide((100, 100), (10, 10), 27, 18) == (0, (424, 424))               # a tie goes to the transformed trial
    assert T.decide((101, 100), (10, 10), 27, 18)[0] == 1
    assert T.decide((0, 500), (40, 3), 27, 0)[0] == 0 and T.decide((0, 500), (40, 3), 27, 7)[0] == 0 and T.decide((0, 500), (40, 3), 27, 8)[0] == 1
    # uint32 arithmetic wraps: 70 * 2^26 = 2^32 + 6 * 2^26
    assert T.decide((5, 5), (40, 3), 27, 1 << 26) == (1, ((5 + (70 << 26)) & 0xFFFFFFFF, (5 + (5 << 26)) & 0xFFFFFFFF))
    assert T.decide((5, 5), (40, 3), 27, -3 & 0xFFFFFFFF)[1][0] == (5 - 210) & 0xFFFFFFFF

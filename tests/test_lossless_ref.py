"""CPU: the composed reference of the lossless entries (tests/lossless_cases.py) -- the committed fixture against a fresh composition,
from the compiled reference where it was built and from the oracle otherwise; bypass and DPCM, which the reference keeps static, on
known answers worked by hand and against the decoder's side; what the fixture must contain."""
import os

import numpy as np
import pytest

import lossless_cases as LC
import oracle_lib as O
import ref_lib as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lossless.npz")
PICS = {p[0]: p for p in LC.FIXTURE_PICTURES}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def fresh():
    """the fixture and its coverage, composed once"""
    return LC.build_fixture(R if R.available() else O)


def test_fixture_regenerates(golden, fresh):
    """from the compiled reference's own kvz_intra_build_reference and kvz_intra_predict where oracle/_ref is built, else from the oracle"""
    assert sorted(golden.files) == sorted(fresh[0])
    for k in golden.files:
        np.testing.assert_array_equal(golden[k], fresh[0][k], err_msg=k)


@pytest.mark.skipif(not R.available(), reason="compiled reference not built")
def test_oracle_and_reference_compose_the_same_fixture(golden):
    d, _ = LC.build_fixture(O)
    for k in golden.files:
        np.testing.assert_array_equal(golden[k], d[k], err_msg=k)


def test_fixture_is_small_numeric_and_covers_every_branch(golden, fresh):
    assert os.path.getsize(GOLDEN) < 400 * 1000
    assert all(golden[k].dtype.kind in "ui" for k in golden.files)
    assert fresh[1] == [], "coverage"
    assert PICS["inter"][1:4] == (72, 72, 1) and PICS["intra"][1:4] == (72, 72, 1) and PICS["mono"][1:4] == (72, 72, 0)
    assert PICS["mixed"][1:4] == (136, 72, 1) and PICS["mixed"][6] == ((0, 1, 2, 3), (0, 1, 2))
    assert PICS["intra"][7] == (0, 1) and PICS["mixed"][7] == (0, 1)
    assert "mono_src_u" not in golden.files
    # the reconstruction of a lossless picture is its source, over every CU an entry handled
    for name, pic in PICS.items():
        case = LC.load_case(golden, pic)
        w, h = case["width"], case["height"]
        done, first = np.zeros(case["cus"].shape, bool), np.zeros(case["cus"].shape, bool)
        for (x, y, s) in LC.RC.inter_cus(case["cus"], w, h):
            done[y // 4:(y + s) // 4, x // 4:(x + s) // 4] = True
            first[y // 4, x // 4] = True
        mid = golden[name + "_mid_rec_y"]
        m = np.kron(done, np.ones((4, 4), bool))
        assert (mid[m] == case["src"][0][m]).all() and (mid[~m] == case["pred"][0][~m]).all(), name
        assert (golden[name + "_mid_costs"][..., 0:2][first] == 0).all()                 # ssd_*: the reconstruction is the source
        assert (golden[name + "_mid_costs"][~first] == LC.RC.POISON_COST).all()
    # implicit_rdpcm matters, in the coefficients and -- through the boundary filter -- in nothing else
    assert not np.array_equal(golden["intra_full0_coeff_y"], golden["intra_full1_coeff_y"])
    np.testing.assert_array_equal(golden["intra_full0_rec_y"], golden["intra_full1_rec_y"])
    np.testing.assert_array_equal(golden["intra_full0_cbf_out"], golden["intra_full1_cbf_out"])


def test_coverage_notices_what_is_missing():
    """the check is not vacuous: a picture of 8x8 inter CUs whose source is its prediction exercises next to nothing"""
    case = LC.fixture_case(("flat", 64, 64, 1, 5, 0.0, None, ()))
    case["cus"]["type"], case["cus"]["depth"], case["cus"]["tr_depth"], case["cus"]["mv_dir"] = LC.IC.CU_INTER, 3, 3, 1
    case["pred"] = case["src"]
    by = {0: LC.compose(case, 0, O)}
    missing = LC.coverage([(case, by, {0: None})])
    assert "inter: plane 0 TU 32" in missing and "inter: plane 0 TU 8" not in missing and "inter: a TU with an all-zero residual" not in missing
    for what in ("intra: plane 0 TU 4", "luma mode 10 on a TU of 16 under implicit_rdpcm", "chroma mode 26 under implicit_rdpcm",
                 "a mode-10 TU whose stored coefficients differ from the plain residual", "a stored |coeff| of 255 made by DPCM",
                 "an NxN CU with four different luma modes and its chroma TUs", "a TU in the ragged right LCU", "a TU in the ragged bottom LCU",
                 "a CU record that would leave the picture", "a luma mode above 34", "a chroma mode above 34",
                 "a luma TU whose prediction differs between implicit_rdpcm 0 and 1", "a TU whose prediction differs from the untiled one"):
        assert what in missing, what


def test_bypass_and_dpcm_known_answers():
    """by hand, from transform.c:73-123"""
    src = np.array([[10, 12, 15, 15], [0, 255, 0, 255], [7, 7, 7, 7], [100, 90, 80, 70]], np.uint8)
    pred = np.full((4, 4), 10, np.uint8)
    c, rec, has = LC.bypass(src, pred)
    assert c.dtype == np.int16 and has == 1 and (rec == src).all()
    assert c.tolist() == [[0, 2, 5, 5], [-10, 245, -10, 245], [-3, -3, -3, -3], [90, 80, 70, 60]]
    # horizontal: the first column stays, every other value loses its left neighbour's ORIGINAL value
    assert LC.rdpcm(c, 10).tolist() == [[0, 2, 3, 0], [-10, 255, -255, 255], [-3, 0, 0, 0], [90, -10, -10, -10]]
    # vertical: the first row stays
    assert LC.rdpcm(c, 26).tolist() == [[0, 2, 5, 5], [-10, 243, -15, 240], [7, -248, 7, -248], [93, 83, 73, 63]]
    # beyond +-255: 255 - 0 against a prediction of 0 next to 0 - 255
    loud = np.array([[0, 255, 0, 255]] * 4, np.uint8)
    c2, _, _ = LC.bypass(loud, np.zeros((4, 4), np.uint8))
    assert LC.rdpcm(c2, 10)[0].tolist() == [0, 255, -255, 255]
    c3, _, _ = LC.bypass(loud, np.array([[0, 0, 255, 0]] * 4, np.uint8))
    assert c3[0].tolist() == [0, 255, -255, 255] and LC.rdpcm(c3, 10)[0].tolist() == [0, 255, -510, 510]
    # no coefficients: has_coeffs 0 and zeros
    z, _, has0 = LC.bypass(src, src)
    assert has0 == 0 and not z.any() and not LC.rdpcm(z, 26).any()
    # the decoder's running sum gives the residual back
    for m in (10, 26):
        assert (LC.decode(pred, LC.rdpcm(c, m), m, 1) == src).all()


def test_decoder_side_identity_over_the_fixture(golden):
    """pred + cumsum(coeff) along the DPCM direction gives back the source for every mode-10 / 26 TU under implicit_rdpcm, pred + coeff
    for every other TU: the stored coefficients are what a decoder needs"""
    B = R if R.available() else O
    seen = {10: 0, 26: 0, "plain": 0}
    for name in ("intra", "mixed", "mono"):
        case = LC.load_case(golden, PICS[name])
        w, h = case["width"], case["height"]
        for r in case["rdpcm"]:
            _, full = LC.compose(case, r, B)
            for t in full["tus"]:
                p, n, x, y = t["plane"], t["n"], t["x"], t["y"]
                sh = 1 if p else 0
                z = LC.RC.xy_to_zorder(32 if p else 64, (x & 63) >> sh, (y & 63) >> sh)
                c = golden["%s_full%d_coeff_%s" % (name, r, "yuv"[p])][(y >> 6) * ((w + 63) // 64) + (x >> 6), z:z + n * n].reshape(n, n)
                pred = np.frombuffer(t["pred"], np.uint8).reshape(n, n)
                back = LC.decode(pred, c, t["mode"], r)
                assert (back == case["src"][p][y >> sh:(y >> sh) + n, x >> sh:(x >> sh) + n]).all(), (name, r, t["plane"], x, y)
                if r and t["mode"] in (10, 26):
                    # what the device relies on, and why no real TU stores more than +-255: the values DPCM changed are differences of
                    # neighbouring source pixels (the prediction is constant along the DPCM direction)
                    s = case["src"][p][y >> sh:(y >> sh) + n, x >> sh:(x >> sh) + n].astype(np.int32)
                    if t["mode"] == 10:
                        assert (c[:, 1:] == np.diff(s, axis=1)).all(), (name, x, y)
                    else:
                        assert (c[1:] == np.diff(s, axis=0)).all(), (name, x, y)
                seen[t["mode"] if (r and t["mode"] in (10, 26)) else "plain"] += 1
    assert min(seen.values()) > 10, seen

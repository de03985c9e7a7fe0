"""CPU: the composed reference of kvz_hip_sao_stats_frame / kvz_hip_sao_frame (tests/sao_frame_cases.py) -- the committed fixture
against a fresh composition from the compiled reference and from the oracle, what the fixture must contain, the candidate arithmetic
against the reference's own ddistortion functions, the band offset that the loop of sao.c:213-222 records, and the reconstruction
composition against a direct per-pixel restatement."""
import os

import numpy as np
import pytest

import oracle_lib as O
import ref_lib as R
import sao_frame_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sao_frame.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")
PICS = SC.FIXTURE_PICTURES
IDS = [p[0] for p in PICS]


def _check_fixture(B):
    z = np.load(GOLDEN, allow_pickle=False)
    fresh, missing = SC.build_fixture(B)
    assert not missing
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)


@needs_ref
def test_fixture_regenerates_from_the_compiled_reference():
    _check_fixture(R)


def test_fixture_regenerates_from_the_oracle():
    _check_fixture(O)


def test_fixture_is_small_numeric_and_holds_the_pictures():
    assert os.path.getsize(GOLDEN) < 600 * 1024
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "ui" for k in z.files)
    assert [(p[0], p[1], p[2], p[3]) for p in PICS] == [("ragged", 200, 136, 1), ("mono", 136, 72, 0), ("one", 64, 64, 1), ("tiny", 8, 8, 1)]
    assert "mono_rec_u" not in z.files and "mono_sao_chroma" not in z.files and z["ragged_dst_y"].shape == (136, 200)
    assert z["ragged_stats"].shape == (36, 104) and z["ragged_cands"].shape == (36, 30) and z["mono_stats"].shape == (6, 104)
    assert SC.STATS.itemsize == 416 and SC.CAND.itemsize == 120
    # the ragged picture's last LCU column is 8 wide and its last row 8 high: 4 x 4 chroma blocks, whose edge tables count 2 x 2 pixels
    assert SC.lcu_blocks(200, 136, 0)[-1] == (192, 128, 8, 8) and SC.lcu_blocks(200, 136, 1)[-1] == (96, 64, 4, 4)
    _, _, _, _, want = SC.load_fixture_case(z, "ragged", 1)
    assert (want["stats"][1:, -1]["edge"][:, :, 1].sum(axis=-1) == 4).all() and (want["stats"][0, -1]["edge"][:, 1].sum(axis=-1) == 36).all()
    assert (want["stats"][0, 0]["band"][1].sum(), want["stats"][1, -1]["band"][1].sum()) == (4096, 16)
    cases = []
    for (name, w, h, chroma, seed) in PICS:
        src, rec, luma, chro, want = SC.load_fixture_case(z, name, chroma)
        cases.append((name, w, h, chroma, rec, luma, chro))
        for k in range(3 if chroma else 1):
            assert not np.array_equal(src[k], rec[k])
            assert {0, 255} <= set(np.unique(rec[k])) or name == "tiny"          # tiny is a single cell of one kind
    assert SC.coverage(cases) == []


@pytest.mark.parametrize("pic", PICS, ids=IDS)
def test_candidate_ddistortion_equals_the_reference_functions(pic):
    """for every (LCU, plane, class): the ddistortion priced from the tables, cnt * o * o - 2 * o * sum, is what sao_edge_ddistortion /
    sao_band_ddistortion compute from the pixels with the recorded offsets"""
    name, w, h, chroma, seed = pic
    B = SC.backend()
    z = np.load(GOLDEN, allow_pickle=False)
    src, rec, _, _, want = SC.load_fixture_case(z, name, chroma)
    nonzero = 0
    for color in range(3 if chroma else 1):
        for i, (x, y, bw, bh) in enumerate(SC.lcu_blocks(w, h, color)):
            o, r = SC.blit(src[color], x, y, bw, bh), SC.blit(rec[color], x, y, bw, bh)
            c = want["cands"][color, i]
            for e in range(4):
                assert c["edge_offsets"][e][0] == 0 and (c["edge_offsets"][e][1:3] >= 0).all() and (c["edge_offsets"][e][3:5] <= 0).all()
                assert c["edge_ddist"][e] == B.sao_edge_ddistortion(o, r, bw, bh, e, c["edge_offsets"][e]), (name, color, i, e)
                nonzero += int(c["edge_ddist"][e] != 0)
            assert 0 <= c["band_position"] <= 27 and (np.abs(c["band_offsets"]) <= 1).all()
            assert c["band_ddist"] == B.sao_band_ddistortion(o, r, bw, bh, int(c["band_position"]), c["band_offsets"]), (name, color, i)
            assert c["band_ddist"] <= 0 and (c["edge_ddist"] <= 0).all()
    assert nonzero or name == "tiny"


def test_band_offset_is_the_last_one_the_loop_visits():
    """one band whose mean error is +5: the loop of sao.c:213-222 walks 5, 4, 3, 2, 1 and, comparing with a best_dist it never updates,
    stores each of them -- what remains is offset 1 and its distortion cnt - 2 * sum, not the minimum at offset 5"""
    rec = np.full((8, 8), 100, np.uint8)                 # band 12
    src = np.full((8, 8), 105, np.uint8)
    band = O.calc_sao_bands(src, rec, 8, 8)
    assert band[1][12] == 64 and band[0][12] == 320 and band[1].sum() == 64
    offs, pos, dist = SC.band_candidate(band)
    assert pos == 9 and list(offs) == [0, 0, 0, 1] and dist == 64 - 2 * 320
    assert dist == SC.backend().sao_band_ddistortion(src, rec, 8, 8, pos, offs)
    assert 64 * 25 - 2 * 5 * 320 < dist                  # the minimum that the comment of :217 intends
    # negative mean error: -1; C's division truncates towards zero: (-3 * 64 + 4 * 64 ... ) stays exact for whole means
    offs, pos, dist = SC.band_candidate(O.calc_sao_bands(np.full((8, 8), 97, np.uint8), rec, 8, 8))
    assert list(offs) == [0, 0, 0, -1] and dist == 64 - 2 * 192
    # truncation: sum -5 over 4 pixels: (-5 + 2) / 4 == 0 in C (floor division would give -1)
    assert SC.c_div(-3, 4) == 0 and SC.c_div(-5, 4) == -1 and SC.c_div(7, 2) == 3
    b = np.zeros((2, 32), np.int32)
    b[0][3], b[1][3] = -5, 4
    assert list(SC.band_candidate(b)[0]) == [0, 0, 0, 0] and SC.band_candidate(b)[2] == 0
    e = np.zeros((4, 2, 5), np.int32)
    e[:, 0, 1:], e[:, 1, 1:] = (-5, 9, 9, -30), (4, 4, 4, 4)          # category 1 truncates to 0, 2 -> +2, 3 positive -> 0, 4 -> -7 (clipped)
    offs, dd = SC.edge_candidate(e)
    assert list(offs[0]) == [0, 0, 2, 0, -7] and dd[0] == (4 * 4 - 2 * 2 * 9) + (4 * 49 - 2 * 7 * 30)


@pytest.mark.parametrize("pic", PICS, ids=IDS)
def test_composition_equals_the_per_pixel_rule(pic):
    name, w, h, chroma, seed = pic
    z = np.load(GOLDEN, allow_pickle=False)
    _, rec, luma, chro, want = SC.load_fixture_case(z, name, chroma)
    direct = SC.direct_recon(rec, luma, chro, chroma)
    for k in range(3 if chroma else 1):
        np.testing.assert_array_equal(direct[k], want["dst"][k], err_msg="%s plane %d" % (name, k))
        assert not np.array_equal(rec[k], want["dst"][k]) or (name == "one" and k == 2)
    if name == "one":
        np.testing.assert_array_equal(rec[2], want["dst"][2])           # V's band position is malformed: a copy


@pytest.mark.parametrize("pic", PICS, ids=IDS)
def test_border_pixels_of_edge_lcus_are_unchanged_and_malformed_records_copy(pic):
    name, w, h, chroma, seed = pic
    z = np.load(GOLDEN, allow_pickle=False)
    _, rec, luma, chro, want = SC.load_fixture_case(z, name, chroma)
    checked = 0
    for color in range(3 if chroma else 1):
        infos = luma if color == 0 else chro
        ph, pw = rec[color].shape
        for i, (x, y, bw, bh) in enumerate(SC.lcu_blocks(w, h, color)):
            eff = SC.effective(infos[i], color)
            got, was = want["dst"][color][y:y + bh, x:x + bw], rec[color][y:y + bh, x:x + bw]
            if eff is None:
                np.testing.assert_array_equal(got, was)
                continue
            if eff[0] != 2:
                continue
            horizontal, vertical = eff[1] != 1, eff[1] != 0
            if horizontal and x == 0:
                np.testing.assert_array_equal(got[:, 0], was[:, 0]); checked += 1
            if horizontal and x + bw == pw:
                np.testing.assert_array_equal(got[:, -1], was[:, -1]); checked += 1
            if vertical and y == 0:
                np.testing.assert_array_equal(got[0], was[0]); checked += 1
            if vertical and y + bh == ph:
                np.testing.assert_array_equal(got[-1], was[-1]); checked += 1
    assert checked or name == "mono"

"""CPU: the composed reference of the four tile entries (tests/tile_chain_cases.py) -- the committed fixture against a fresh composition
from the compiled reference and from the oracle; what the fixture must contain; a grid of one tile composes to the untiled compositions;
and the stages that do not depend on tiles compose to the same values tile by tile and over the whole picture."""
import os

import numpy as np
import pytest

import inter_residual_cases as RC
import lcu_qp_cases as QC
import oracle_lib as O
import ref_lib as R
import sao_frame_cases as SC
import tile_chain_cases as TC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_chain.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")
RAGGED = TC.FIXTURE_PICTURES[0]


@pytest.fixture(scope="module")
def fresh():
    """the fixture and its coverage from the oracle, composed once"""
    return TC.build_fixture(O)


def _same(z, d):
    assert sorted(z.files) == sorted(d)
    for k in z.files:
        np.testing.assert_array_equal(z[k], d[k], err_msg=k)


@needs_ref
def test_fixture_regenerates_from_the_compiled_reference():
    d, missing = TC.build_fixture(R)
    assert not missing
    _same(np.load(GOLDEN, allow_pickle=False), d)


def test_fixture_regenerates_from_the_oracle(fresh):
    _same(np.load(GOLDEN, allow_pickle=False), fresh[0])


def test_fixture_is_small_numeric_and_covers_every_boundary_rule(fresh):
    assert os.path.getsize(GOLDEN) < 600 * 1000
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "ui" for k in z.files)
    assert fresh[1] == [], "coverage"
    pics = {p[0]: p for p in TC.FIXTURE_PICTURES}
    assert pics["ragged"][1:4] == (200, 136, 1) and pics["ragged"][9:] == ((0, 1, 4), (0, 2, 3)) and pics["ragged"][4:6] == (1, 0)
    assert pics["columns"][1:4] == (192, 64, 1) and pics["columns"][9:] == ((0, 1, 2, 3), (0, 1)) and pics["columns"][5] == 1
    assert pics["mono"][1:4] == (96, 72, 0) and pics["mono"][9:] == ((0, 1, 2), (0, 1, 2)) and "mono_rec_u" not in z.files
    assert [t[:4] for t in TC.tiles(200, 136, (0, 1, 4), (0, 2, 3))] == [(0, 0, 64, 128), (64, 0, 200, 128), (0, 128, 64, 136), (64, 128, 200, 136)]
    cus = np.ascontiguousarray(z["columns_cus"]).view(TC.CU_INFO)
    assert (cus["type"] == 1).all(), "columns is all intra"
    ragged = np.ascontiguousarray(z["ragged_cus"]).view(TC.CU_INFO)
    assert 0.3 < (ragged["type"] == 1).mean() < 0.6
    assert 22 <= z["ragged_lcu_qp"].min() and z["ragged_lcu_qp"].max() <= 42 and len(set(z["ragged_lcu_qp"].tolist())) > 6


def test_coverage_notices_what_is_missing():
    """the check is not vacuous: with one tile no boundary rule is exercised, and each stage is reported"""
    case = TC.fixture_case(*TC.FIXTURE_PICTURES[2])
    plain = dict(case)
    plain["col_bd"], plain["row_bd"] = TC.one_tile(case["width"], case["height"])
    chain = TC.compose_chain(plain, O)
    missing = TC.coverage([plain], [chain], [chain])
    for stage in ("intra: a luma TU at the left edge", "intra: tiled != untiled next to a vertical", "deblocking: a luma edge on a vertical",
                  "SAO: an edge record of class 0 in an LCU at a horizontal", "SAO: a boundary pixel of class 2", "QP map: a tile whose first LCU"):
        assert any(m.startswith(stage) for m in missing), stage


def test_one_tile_composes_to_the_untiled_compositions():
    case = TC.fixture_case(*RAGGED)
    w, h, chroma = case["width"], case["height"], case["chroma"]
    got = TC.compose_chain(case, O, TC.one_tile(w, h))
    init = QC.zero_outputs(w, h, chroma)
    _, full, mapped, last = QC.compose_chain(case["src"], case["pred"], case["cus"], case["modes"], case["lcu_qp"], case["start_qp"], 0, chroma,
                                             case["signhide"], case["slice_is_intra"], B=O, init=init)
    QC.assert_outputs_equal(got["full"], full, "intra", chroma)
    np.testing.assert_array_equal(got["cus_qp"].view(np.uint8), mapped.view(np.uint8))
    np.testing.assert_array_equal(got["last"], last)
    rows, last_rows = QC.set_cu_qps(full["cus"], full["cbf_out"], case["lcu_qp"], case["start_qp"], QC.lcu_grid(w, h)[0])
    np.testing.assert_array_equal(got["cus_qp_rows"].view(np.uint8), rows.view(np.uint8))
    np.testing.assert_array_equal(got["last_rows"], last_rows)
    deb = O.deblock_frame(full["rec"][0], full["rec"][1], full["rec"][2], mapped, TC.chain_deblock_params(case))
    dst = SC.compose_recon(deb, case["sao_luma"], case["sao_chroma"], chroma, O)
    for k in range(3):
        np.testing.assert_array_equal(got["deb"][k], deb[k])
        np.testing.assert_array_equal(got["sao"][k], dst[k])
    # and the tiles matter: the fixture's grid gives other pictures at every stage
    tiled = TC.compose_chain(case, O)
    assert not np.array_equal(tiled["full"]["rec"][0], got["full"]["rec"][0]) and not np.array_equal(tiled["last"], got["last"])
    assert not np.array_equal(tiled["deb"][1], got["deb"][1]) and not np.array_equal(tiled["sao"][0], got["sao"][0])


def test_stages_without_tile_rules_compose_alike_per_tile_and_per_picture():
    """kvz_hip_inter_residual_frame (per TU) and kvz_hip_sao_stats_frame (LCU interiors) on `ragged`"""
    case = TC.fixture_case(*RAGGED)
    w, h, chroma = case["width"], case["height"], case["chroma"]
    init = RC.initial_outputs(w, h, chroma)
    for qp in (24, 39):
        whole = RC.compose(case["src"], case["pred"], case["cus"], qp, chroma, case["signhide"], B=O, init=init)
        parts = TC.inter_residual(case["src"], case["pred"], case["cus"], qp, case["col_bd"], case["row_bd"], chroma, case["signhide"], B=O, init=init)
        RC.assert_outputs_equal(parts, whole, "inter residual qp %d" % qp, chroma)
    z = np.load(GOLDEN, allow_pickle=False)
    deb = tuple(z["ragged_deb_" + n] for n in "yuv")
    np.testing.assert_array_equal(TC.sao_stats(case["src"], deb, case["col_bd"], case["row_bd"], chroma, O).view(np.int32),
                                  SC.compose_stats(case["src"], deb, chroma, O).view(np.int32))


def test_uniform_spacing_is_the_reference_formula():
    assert TC.uniform_bd(30, 4) == [0, 7, 15, 22, 30] and TC.uniform_bd(17, 2) == [0, 8, 17] and TC.uniform_bd(5, 5) == [0, 1, 2, 3, 4, 5]
    from kvazaar_amd import api
    g = api.uniform_tile_grid(1920, 1080, 4, 2)
    assert (int(g["cols"][0]), int(g["rows"][0])) == (4, 2)
    assert g["col_bd"][0, :5].tolist() == [0, 7, 15, 22, 30] and g["row_bd"][0, :3].tolist() == [0, 8, 17]
    assert not g["col_bd"][0, 5:].any() and not g["row_bd"][0, 3:].any()
    h = api.tile_grid(200, 136, [0, 1, 4], [0, 2, 3])
    assert h["col_bd"][0, :3].tolist() == [0, 1, 4] and h["row_bd"][0, :3].tolist() == [0, 2, 3] and h.nbytes == 392

"""CPU: the composed reference of the per-LCU-QP entries (tests/lcu_qp_cases.py) -- with a uniform QP array it is the existing
composition of both case modules; the committed fixture against a fresh composition from the compiled reference and from the oracle; what
the fixture must contain; the known answers of the QP map against the restated set_cu_qps; and the composed map through the deblocking
filter of the reference with per_cu_qp = 1."""
import os

import numpy as np
import pytest

import inter_residual_cases as RC
import intra_recon_cases as XC
import lcu_qp_cases as QC
import oracle_lib as O
import ref_lib as R
from patterns import deblock_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lcu_qp.npz")
INTRA_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "intra_recon.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")


@pytest.mark.parametrize("pic", QC.FIXTURE_PICTURES[:2], ids=[p[0] for p in QC.FIXTURE_PICTURES[:2]])
def test_uniform_array_is_the_existing_composition_of_both_stages(pic):
    name, w, h, chroma, signhide, slice_is_intra = pic[:6]
    src, pred, cus, modes = QC.fixture_case(*pic)
    n = len(pic[9])
    for qp in (22, 37):
        init = RC.initial_outputs(w, h, chroma)
        a = QC.compose_inter(src, pred, cus, [qp] * n, chroma, signhide, slice_is_intra, B=O, init=init)
        b = RC.compose(src, pred, cus, qp, chroma, signhide, slice_is_intra, B=O, init=init)
        RC.assert_outputs_equal(a, b, "%s inter qp %d" % (name, qp), chroma)
        assert [t[:3] for t in a["tus"]] == b["tus"] and {t[3] for t in a["tus"]} == {qp}
        nxt = (b["coeff"], b["cbf_out"], b["costs"])
        c = QC.compose_intra(src, b["rec"], b["cus"], modes, [qp] * n, chroma, signhide, slice_is_intra, B=O, init=nxt)
        d = XC.compose(src, b["rec"], b["cus"], modes, qp, chroma, signhide, slice_is_intra, B=O, init=nxt)
        XC.assert_outputs_equal(c, d, "%s intra qp %d" % (name, qp), chroma)
        assert [t[:9] for t in c["tus"]] == d["tus"]


def test_out_of_range_values_compose_as_0_and_51():
    pic = QC.FIXTURE_PICTURES[1]
    name, w, h, chroma, signhide, slice_is_intra = pic[:6]
    src, pred, cus, modes = QC.fixture_case(*pic)
    a = QC.compose_inter(src, pred, cus, [-3, 60, -128, 127], chroma, signhide, slice_is_intra, B=O)
    b = QC.compose_inter(src, pred, cus, [0, 51, 0, 51], chroma, signhide, slice_is_intra, B=O)
    RC.assert_outputs_equal(a, b, name, chroma)


def _check_fixture(B):
    z = np.load(GOLDEN, allow_pickle=False)
    fresh, missing = QC.build_fixture(B)
    assert not missing
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)


@needs_ref
def test_fixture_regenerates_from_the_compiled_reference():
    _check_fixture(R)


def test_fixture_regenerates_from_the_oracle():
    _check_fixture(O)


def test_fixture_is_small_numeric_and_covers_what_the_entries_must_handle():
    assert os.path.getsize(GOLDEN) <= os.path.getsize(INTRA_GOLDEN)
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "ui" for k in z.files)
    pics = {p[0]: p for p in QC.FIXTURE_PICTURES}
    assert pics["ragged"][1:4] == (200, 136, 1) and pics["mono"][1:4] == (96, 72, 0)
    assert len(set(pics["ragged"][9][:4])) == 4, "the four LCUs of the first row differ: one N = 4 workgroup spans them"
    assert "mono_rec_u" not in z.files and z["ragged_rec_y"].shape == (136, 200)
    inter, intra, qps = [], [], []
    for pic in QC.FIXTURE_PICTURES:
        name, chroma = pic[0], pic[3]
        qps += z[name + "_lcu_qp"].tolist()
        assert z[name + "_lcu_qp"].dtype == np.int8 and z[name + "_lcu_qp"].tolist() == list(pic[9])
        if chroma:
            inter += [tuple(int(v) for v in t) for t in z[name + "_inter_tus"]]
            intra += [tuple(int(v) for v in t) for t in z[name + "_intra_tus"]]
    assert QC.coverage(inter, intra, qps) == []
    # the check itself notices what is missing
    assert "QP 51" in QC.coverage(inter, intra, [q for q in qps if q != 51])
    assert any("residue 5" in m for m in QC.coverage(inter, intra, [q for q in qps if q % 6 != 5]))
    assert any("at or above 43" in m for m in QC.coverage(inter, intra, [q for q in qps if q < 43] + [51 - 6 * 6]))
    assert "inter plane 0 size 32 has_coeffs 1 under two QPs" in QC.coverage([t for t in inter if t[3] != 10], intra, qps) + \
        QC.coverage([t for t in inter if t[1] != 32], intra, qps)
    assert any(m.startswith("intra plane 1 size 16") for m in QC.coverage(inter, [t for t in intra if not (t[0] == 1 and t[1] == 16)], qps))
    assert QC.coverage(inter, intra, qps, known=QC.KNOWN_CASES[:-1]) == ["QP map: " + QC.KNOWN_CASES[-1]]
    # the QP map of the fixture is not trivial: SCUs that carry the predictor and not their LCU's QP, and chains that differ
    for name in ("ragged", "coarse"):
        w, h = pics[name][1:3]
        own = np.kron(QC.clip_qp(pics[name][9]).reshape(QC.lcu_grid(w, h)[::-1]), np.ones((16, 16), np.int64))[:h // 4, :w // 4]
        got = z[name + "_cus_qp"][:, :, 6]
        assert (got != own).any() and (got == own).any()
    assert not np.array_equal(z["ragged_last"], z["ragged_last_rows"])


def test_known_answers_of_the_qp_map():
    """an LCU whose first CU is coded, one whose first coded CU is in the middle, one with none, two uncoded LCUs in a row, a chain start,
    chain_lcus 0 against row chains, ragged right and bottom LCUs: tables written by hand in lcu_qp_cases"""
    cus, cbf, one_chain, row_chains = QC.known_map()
    lx, ly = QC.lcu_grid(QC.KNOWN_W, QC.KNOWN_H)
    assert (lx, ly) == (4, 3) and QC.KNOWN_W % 64 and QC.KNOWN_H % 64
    firsts = [f for (_, f) in QC.KNOWN_LCUS]
    assert firsts[0] == 0 and firsts[1] not in (0, None) and firsts[2] is None and firsts[4] is None and firsts[5] is None
    assert QC.KNOWN_LAST_ONE_CHAIN[0] == QC.KNOWN_START and QC.KNOWN_LAST_ROW_CHAINS[4] == QC.KNOWN_START != QC.KNOWN_LAST_ONE_CHAIN[4]
    for chain, want, last in ((0, one_chain, QC.KNOWN_LAST_ONE_CHAIN), (lx, row_chains, QC.KNOWN_LAST_ROW_CHAINS)):
        got, got_last = QC.set_cu_qps(cus, cbf, QC.KNOWN_LCU_QP, QC.KNOWN_START, chain)
        np.testing.assert_array_equal(got["qp"], want, err_msg="chain_lcus %d" % chain)
        assert got_last.tolist() == list(last) and got_last.dtype == np.int8
        # nothing but qp moved
        got["qp"] = cus["qp"]
        np.testing.assert_array_equal(got.view(np.uint8), cus.view(np.uint8))
    # a chain of two rows: the second row continues, the third starts again
    _, last = QC.set_cu_qps(cus, cbf, QC.KNOWN_LCU_QP, QC.KNOWN_START, 2 * lx)
    assert last.tolist() == list(QC.KNOWN_LAST_ONE_CHAIN[:8]) + list(QC.KNOWN_LAST_ROW_CHAINS[8:])


def test_the_walk_reads_depth_above_3_as_3_and_no_type():
    cus, cbf, one_chain, _ = QC.known_map()
    other = np.array(cus)
    other["depth"][other["depth"] == 3] = 200
    other["type"] = 0
    got, _ = QC.set_cu_qps(other, cbf, QC.KNOWN_LCU_QP, QC.KNOWN_START, 0)
    np.testing.assert_array_equal(got["qp"], one_chain)


def test_composed_map_deblocks_alike_in_reference_and_oracle_with_per_cu_qp():
    """the chain's picture: no blank records, which the reference's filter cannot take (lcu_qp_cases.chain_case)"""
    w, h, start_qp = 200, 136, 31
    src, pred, cus, modes, lcu_qp = QC.chain_case(w, h, 2000)
    assert len(set(lcu_qp.tolist())) > 8
    _, full, mapped, _ = QC.compose_chain(src, pred, cus, modes, lcu_qp, start_qp, 0, B=O, init=QC.zero_outputs(w, h, 1))
    own = np.kron(QC.clip_qp(lcu_qp).reshape(3, 4), np.ones((16, 16), np.int64))[:h // 4, :w // 4]
    assert (mapped["qp"] != own).any(), "some SCUs carry the predictor"
    y, u, v = full["rec"]
    prm = deblock_params(qp=start_qp, per_cu_qp=1)
    a = O.deblock_frame(y, u, v, mapped, prm)
    assert not np.array_equal(a[0], y) and not np.array_equal(a[1], u)
    assert not np.array_equal(O.deblock_frame(y, u, v, mapped, deblock_params(qp=start_qp, per_cu_qp=0))[0], a[0]), "the map matters"
    other = np.array(mapped)
    other["qp"] = own
    assert not np.array_equal(O.deblock_frame(y, u, v, other, prm)[0], a[0]), "the predicted QPs matter"
    if R.available():
        b = R.deblock_frame(y, u, v, mapped, prm)
        for k in range(3):
            np.testing.assert_array_equal(a[k], b[k])

"""CPU: the composed reference of the scaling-list entries (tests/scaling_list_cases.py) -- the committed fixture against a fresh
composition; the restated list processing against the compiled reference's processed tables; what the fixture must contain."""
import os

import numpy as np
import pytest

import oracle_lib as O
import ref_lib as R
import scaling_list_cases as SL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaling_list.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def fresh(golden):
    """the fixture and its coverage from the oracle, composed once; the default lists are the tables recorded from the reference"""
    return SL.build_fixture(O, default_tables=SL.undense(golden["default_quant"], golden["default_dequant"]))


def _same(z, d, keys=None):
    keys = sorted(z.files) if keys is None else keys
    assert keys == sorted(k for k in d if keys is None or k in keys)
    for k in keys:
        np.testing.assert_array_equal(z[k], d[k], err_msg=k)


@needs_ref
def test_default_list_pictures_regenerate_from_the_compiled_reference(golden):
    """through the reference's own kvz_quantize_residual with its default scaling lists (sl = 1), tables and all"""
    d, _ = SL.build_fixture(R, sets=("default",), probe=False)
    keys = sorted(k for k in golden.files if "_custom_" not in k and "_chain_" not in k and not k.startswith("custom_"))
    assert any("_default_full_coeff_y" in k for k in keys) and "default_quant" in keys
    _same(golden, {k: d[k] for k in keys}, keys)


def test_fixture_regenerates_from_the_oracle(golden, fresh):
    """default-list and custom-list pictures alike, through the oracle's table path"""
    _same(golden, fresh[0])


def test_fixture_is_small_numeric_and_covers_every_branch(golden, fresh):
    assert os.path.getsize(GOLDEN) < 600 * 1000
    assert all(golden[k].dtype.kind in "ui" for k in golden.files)
    assert fresh[1] == [], "coverage"
    pics = {p[0]: p for p in SL.FIXTURE_PICTURES}
    assert pics["hide"][1:5] == (128, 128, 1, 1) and pics["hide"][9] is None
    assert pics["ragged"][1:4] == (200, 136, 1) and len(pics["ragged"][9]) == 12 and pics["ragged"][10] == ((0, 2, 4), (0, 1, 3))
    assert {22, 51} <= set(pics["ragged"][9])
    assert pics["mono"][1:4] == (96, 72, 0) and "mono_src_u" not in golden.files
    # the custom set: U and V differ, entries of 1..4, distinct DC values for 16x16 and 32x32
    c = [golden["custom_coeff_%d" % s] for s in range(4)]
    assert [a.shape for a in c] == [(6, 16), (6, 64), (6, 64), (2, 64)]
    assert all(not np.array_equal(a[b + 1], a[b + 2]) for a in c[:3] for b in (0, 3))
    assert all(((a >= 1) & (a <= 4)).any() and a.min() >= 1 for a in c)
    dc = golden["custom_dc"]
    assert len(set(dc[2].tolist())) == 6 and dc[3, 0] != dc[3, 1] and (dc[2] > 0).all() and (dc[3, :2] > 0).all()
    # and the lists matter: the two sets give different pictures
    assert not np.array_equal(golden["hide_default_full_rec_y"], golden["hide_custom_full_rec_y"])
    assert not np.array_equal(golden["mono_default_mid_coeff_y"], golden["mono_custom_mid_coeff_y"])


def test_coverage_notices_what_is_missing():
    """the check is not vacuous: the log of one picture at one low QP lacks the left-shift branch and more"""
    case = SL.fixture_case(SL.FIXTURE_PICTURES[0])
    B = SL.Listed(O, SL.process_lists(*SL.custom_lists()), probe=True)
    SL.compose(case, B)
    missing = SL.coverage(B.log)
    for what in ("inter size 32 with coefficients in dequantisation branch 2", "intra size 4 with coefficients in dequantisation branch 2",
                 "inter: a coefficient with |coef| * factor >= 2^32"):
        assert what in missing, what
    assert SL.coverage([]) and len(SL.coverage([])) > 50


def test_large_product_is_real():
    """a 32x32 TU whose source is its prediction + 120 has a DC coefficient near 15000 (the oracle's forward transform), and with a DC
    list entry of 1 the factor is 26214 << 4 at rem 0: the product needs more than 32 bits"""
    coef = O.transform_batch("dct", 32, np.full((1, 1024), 120, np.int16)).astype(np.int64)
    assert 15000 <= coef[0, 0] <= 15400 and not coef[0, 1:].any()
    t = SL.process_lists(*SL.custom_lists())
    q = t[(3, 3, 0)][0]
    assert q[0] == 26214 << 4 and int(coef[0, 0]) * int(q[0]) >= 2 ** 32


@needs_ref
def test_restated_list_processing_reproduces_the_reference_tables(golden):
    """process_lists against ref_lib.scaling_tables for every size, list and remainder, starting from the default lists recovered as
    dequant[rem 0] / 40.  This, with the oracle-vs-reference tests of the table path (tests/test_oracle_vs_ref.py), is what the
    custom-list expectations rest on: the reference harness cannot load custom lists, and oracle/ is not to change."""
    ref = SL.reference_default_tables()
    coeff, dc = SL.lists_from_tables(ref)
    assert not dc.any() or set(np.unique(dc)) <= {0, 16}
    mine = SL.process_lists(coeff, dc)
    assert sorted(mine) == sorted(ref) and len(ref) == 3 * 36 + 3 * 6
    for key in ref:
        np.testing.assert_array_equal(mine[key][0], ref[key][0], err_msg="quant %s" % (key,))
        np.testing.assert_array_equal(mine[key][1], ref[key][1], err_msg="dequant %s" % (key,))
    q, d = SL.dense(ref)
    np.testing.assert_array_equal(q, golden["default_quant"])
    np.testing.assert_array_equal(d, golden["default_dequant"])
    # the default 8x8 lists are not flat, so the recovery is not vacuous
    assert coeff[1][0].max() == 115 and coeff[1][3].max() == 91 and (coeff[0] == 16).all()


def test_dc_and_upsampling_of_the_restated_processing():
    """known answers by hand: a 16x16 table repeats each list coefficient 2x2 and takes the DC value at [0]; a 4x4 table has no DC"""
    coeff, dc = SL.custom_lists()
    t = SL.process_lists(coeff, dc)
    q, d = t[(2, 4, 3)]
    c = coeff[2][4].reshape(8, 8)
    assert d[0] == 57 * dc[2][4] and q[0] == (18396 << 4) // dc[2][4]
    assert d.reshape(16, 16)[5, 9] == 57 * c[2, 4] and q.reshape(16, 16)[15, 14] == (18396 << 4) // c[7, 7] and d[1] == 57 * c[0, 0]
    q4, d4 = t[(0, 2, 5)]
    assert d4[0] == 72 * coeff[0][2][0] and q4[7] == (14564 << 4) // coeff[0][2][7]
    assert t[(3, 3, 1)][0] is t[(3, 1, 1)][0] and (3, 2, 0) not in t

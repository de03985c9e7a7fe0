"""CPU: the composed motion-compensation reference of tests/inter_recon_cases.py against the reference's own
kvz_inter_recon_bipred (through ref_lib.bipred_luma_satd, which returns its luma prediction), and the committed fixture
tests/golden/inter_recon.npz against a fresh composition."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import inter_recon_cases as IC
import oracle_lib as O
import ref_lib as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_recon.npz")
W, H = 128, 128
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")


@contextlib.contextmanager
def generic_blend():
    """kvz_inter_recon_bipred blends through the selector's global kvz_inter_recon_bipred_blend.  The semantics to pin are the
    generic strategy's, so that one pointer is set to the generic function for the comparison and put back afterwards: the avx2
    blend the selector picks on this kind of host returns 255 for some widths (24, 48, 64) when both vectors are integer
    (its no-mov path), which is not what an encoder without avx2 -- or the GPU -- computes."""
    L = R.lib()
    ptr = ctypes.c_void_p.in_dll(L, "kvz_inter_recon_bipred_blend")
    old = ptr.value
    ptr.value = L.ref_strategy(b"inter_recon_bipred", b"generic")
    try:
        yield
    finally:
        ptr.value = old


def _planes():
    g = np.random.default_rng(77)
    return [g.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3)]


def _positions(w, h):
    """the four corners of the picture and an interior position; a PU never crosses an LCU (the reference addresses it inside lcu_t)"""
    return sorted({(0, 0), (W - w, 0), (0, H - h), (W - w, H - h), (64 - w, 64 - h)})


# integer / half / quarter combinations of the two vectors, near the block
NEAR = [((0, 0), (0, 0)), ((4, -8), (2, 0)), ((0, 2), (-12, 4)), ((1, 3), (2, 2)), ((-5, 6), (7, -9)), ((2, 2), (0, 0)), ((3, 0), (0, 1)),
        ((-16, 20), (-2, -2))]
# windows partly and wholly outside on every side and corner
FAR = [((-4 * (W + 10), 3), (5, 4 * (H + 20))), ((4 * (W + 10) + 1, -6), (0, -4 * (H + 10))), ((-4 * (W + 70) + 2, -4 * (H + 70) + 1), (4 * (W + 70), 4 * (H + 70) + 2)),
       ((4 * (W + 30), -4 * (H + 30) + 3), (-4 * (W + 30) + 1, 4 * (H + 30))), ((-9, -11), (4 * W - 6, 4 * H - 2)), ((-4 * 3 - 1, -4 * 2 - 2), (13, 9))]


@needs_ref
def test_composed_bipred_luma_equals_kvz_inter_recon_bipred():
    pic, ref0, ref1 = _planes()
    refs = [(ref0, None, None), (ref1, None, None)]
    n = 0
    for (w, h) in IC.PU_SHAPES:
        for (x, y) in _positions(w, h):
            for (mv0, mv1) in NEAR + FAR:
                with generic_blend():
                    _, want = R.bipred_luma_satd(pic, ref0, ref1, x, y, w, h, mv0, mv1)
                pu = IC.make_pu(x, y, w, h, 3, mv0, mv1, 0, 1)
                for B in (R, O):
                    got = IC.predict_pu(refs, pu, chroma=0, B=B)[0]
                    np.testing.assert_array_equal(got, want, err_msg="%dx%d at (%d,%d) mv %s %s" % (w, h, x, y, mv0, mv1))
                n += 1
    assert n >= 24 * 4 * 14


@needs_ref
def test_identical_halves_equal_the_composed_uniprediction():
    """(2 s + 64) >> 7 == (s + 32) >> 6: kvz_inter_recon_bipred with the same picture and vector twice pins the 8-bit path"""
    pic, ref0, _ = _planes()
    refs = [(ref0, None, None)]
    for (w, h) in IC.PU_SHAPES:
        for (x, y) in _positions(w, h):
            for (mv, _) in NEAR + FAR:
                with generic_blend():
                    _, want = R.bipred_luma_satd(pic, ref0, ref0, x, y, w, h, mv, mv)
                for B in (R, O):
                    got = IC.predict_pu(refs, IC.make_pu(x, y, w, h, 1, mv), chroma=0, B=B)[0]
                    np.testing.assert_array_equal(got, want, err_msg="%dx%d at (%d,%d) mv %s" % (w, h, x, y, mv))


def test_pu_shapes_are_the_24_of_the_inter_search():
    assert len(IC.PU_SHAPES) == 24 and (4, 8) in IC.PU_SHAPES and (64, 48) in IC.PU_SHAPES and (12, 16) in IC.PU_SHAPES
    assert all(IC.shape_ok(w, h) for (w, h) in IC.PU_SHAPES) and not IC.shape_ok(4, 4) and not IC.shape_ok(12, 12)


def test_walk_covers_every_part_mode_and_the_maps_are_consistent():
    cus, ref_LX = IC.random_cu_map(256, 192, 5, n_refs=3, slice_b=True)
    pus = IC.walk_pus(cus, ref_LX, 256, 192)
    inter = cus["type"] == IC.CU_INTER
    assert set(np.unique(cus["part_size"][inter])) == set(range(8)) and set(np.unique(cus["depth"][inter])) == {0, 1, 2, 3}
    assert (cus["type"] == IC.CU_INTRA).any() and (cus["type"] == 0).any() and set(np.unique(pus["mv_dir"])) == {1, 2, 3}
    # valid PUs tile the inter area without overlap
    cover = np.zeros((192, 256), dtype=np.int32)
    for p in pus:
        if IC.pu_valid(p, 256, 192, 3):
            cover[p["y"]:p["y"] + p["height"], p["x"]:p["x"] + p["width"]] += 1
    assert cover.max() == 1
    assert not (cover.astype(bool) & ~np.kron(inter, np.ones((4, 4), dtype=bool))).any()


def _check_fixture(B):
    z = np.load(GOLDEN, allow_pickle=False)
    fresh = IC.build_fixture(B)
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)


@needs_ref
def test_fixture_regenerates_from_the_compiled_reference():
    _check_fixture(R)


def test_fixture_regenerates_from_the_oracle():
    _check_fixture(O)


def test_fixture_is_small_and_numeric():
    assert os.path.getsize(GOLDEN) < 600 * 1024
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "ui" for k in z.files)
    names = [c[0] for c in IC.FIXTURE_PICTURES]
    assert names == ["ragged", "b4", "mono"] and "mono_want_u" not in z.files and z["ragged_want_y"].shape == (136, 200)

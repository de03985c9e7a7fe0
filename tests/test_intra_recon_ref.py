"""CPU: the composed reference of kvz_hip_intra_recon_frame (tests/intra_recon_cases.py) -- the committed fixture against a fresh
composition from the compiled reference and from the oracle, what the fixture must contain, that the walk covers the intra CUs exactly
once, that the composition never reads what the intra CUs held on entry, and the composed flags through both deblocking filters."""
import os

import numpy as np
import pytest

import inter_recon_cases as IC
import inter_residual_cases as RC
import intra_recon_cases as XC
import oracle_lib as O
import ref_lib as R
from patterns import deblock_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra_recon.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")


def _check_fixture(B):
    z = np.load(GOLDEN, allow_pickle=False)
    fresh, missing = XC.build_fixture(B)
    assert not missing
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)


@needs_ref
def test_fixture_regenerates_from_the_compiled_reference():
    _check_fixture(R)


def test_fixture_regenerates_from_the_oracle():
    _check_fixture(O)


def test_fixture_is_small_numeric_and_covers_what_the_entry_must_handle():
    assert os.path.getsize(GOLDEN) < 600 * 1024
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "ui" for k in z.files)
    pics = {p[0]: p for p in XC.FIXTURE_PICTURES}
    assert pics["ragged"][1:4] == (200, 136, 1) and pics["full"][1:4] == (256, 192, 1) and pics["mono"][1:4] == (128, 128, 0)
    assert {p[5] for p in pics.values()} == {0, 1} and {p[6] for p in pics.values()} == {0, 1} and len({p[4] for p in pics.values()}) == 2
    assert "mono_rec_u" not in z.files and z["ragged_rec_y"].shape == (136, 200)
    tus, maps = [], []
    for pic in XC.FIXTURE_PICTURES:
        name, w, h, chroma = pic[:4]
        _, _, cus, modes, _ = XC.load_fixture_case(z, name, chroma)
        typ = set(np.unique(cus["type"]).tolist())
        assert typ == ({IC.CU_INTRA} if name == "full" else {0, IC.CU_INTRA, IC.CU_INTER}), name
        if chroma:
            tus += [tuple(int(v) for v in t) for t in z[name + "_tus"]]
            maps.append((cus, modes, w, h))
    assert XC.coverage(tus, maps) == []
    # the check itself notices a population that lacks something
    assert "luma TU 32" in XC.coverage([t for t in tus if t[1] != 32], maps)
    assert any("above-right" in m for m in XC.coverage([t for t in tus if t[6] % 64], maps))


@pytest.mark.parametrize("pic", XC.FIXTURE_PICTURES, ids=[p[0] for p in XC.FIXTURE_PICTURES])
def test_walk_covers_every_intra_pixel_once_and_nothing_else(pic):
    name, w, h, chroma = pic[:4]
    _, _, cus, modes = XC.fixture_case(*pic)
    m, mc, _ = XC.intra_mask(cus, w, h)
    count = [np.zeros((h, w), np.int32), np.zeros((h // 2, w // 2), np.int32), np.zeros((h // 2, w // 2), np.int32)]
    done = np.zeros((h, w), bool)
    for (p, x, y, n, cu_x, cu_y, mode, scan, leaf) in XC.walk_tus(cus, modes, w, h, chroma):
        sh = 1 if p else 0
        count[p][y >> sh:(y >> sh) + n, x >> sh:(x >> sh) + n] += 1
        assert mode == modes[y // 4, x // 4, 1 if p else 0]
        assert leaf == 64 >> min(4, max(int(cus[cu_y // 4, cu_x // 4]["depth"]), int(cus[y // 4, x // 4]["tr_depth"]), 1))
        if p == 0:
            # coding order: the intra pixels right beside and above the TU were walked before it
            if x:
                assert (done[y:y + n, x - 1] | ~m[y:y + n, x - 1]).all()
            if y:
                assert (done[y - 1, x:x + n] | ~m[y - 1, x:x + n]).all()
            done[y:y + n, x:x + n] = True
    assert (count[0][m] == 1).all() and (count[0][~m] == 0).all()
    for p in (1, 2) if chroma else ():
        assert (count[p][mc] == 1).all() and (count[p][~mc] == 0).all()


@pytest.mark.parametrize("pic", XC.FIXTURE_PICTURES[:3], ids=[p[0] for p in XC.FIXTURE_PICTURES[:3]])
def test_composition_does_not_depend_on_what_the_intra_cus_held(pic):
    name, w, h, chroma, qp, signhide, slice_is_intra = pic[:7]
    src, rec, cus, modes = XC.fixture_case(*pic)
    other = XC.poison_intra(rec, cus, 999, chroma)
    assert not np.array_equal(other[0], rec[0])
    init = RC.initial_outputs(w, h, chroma)
    a = XC.compose(src, rec, cus, modes, qp, chroma, signhide, slice_is_intra, B=O, init=init)
    b = XC.compose(src, other, cus, modes, qp, chroma, signhide, slice_is_intra, B=O, init=init)
    XC.assert_outputs_equal(a, b, name, chroma)
    # and nothing outside the intra CUs moved
    m, mc, ms = XC.intra_mask(cus, w, h)
    for k in range(3 if chroma else 1):
        np.testing.assert_array_equal(a["rec"][k][~(mc if k else m)], rec[k][~(mc if k else m)])
    assert (a["cbf_out"][~ms] == RC.POISON_CBF).all()
    np.testing.assert_array_equal(a["cus"][~ms].view(np.uint8), cus[~ms].view(np.uint8))


@pytest.mark.parametrize("pic", XC.FIXTURE_PICTURES, ids=[p[0] for p in XC.FIXTURE_PICTURES])
def test_composed_flags_deblock_alike_in_reference_and_oracle(pic):
    name, w, h, chroma, qp = pic[:5]
    z = np.load(GOLDEN, allow_pickle=False)
    _, _, _, _, want = XC.load_fixture_case(z, name, chroma)
    prm = deblock_params(qp=qp, chroma=chroma)
    y, u, v = want["rec"]
    a = O.deblock_frame(y, u, v, want["cus"], prm)
    assert not np.array_equal(a[0], y)
    if R.available():
        b = R.deblock_frame(y, u, v, want["cus"], prm)
        for k in range(3 if chroma else 1):
            np.testing.assert_array_equal(a[k], b[k])

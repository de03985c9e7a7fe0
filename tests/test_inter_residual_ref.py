"""CPU: the composed reference of kvz_hip_inter_residual_frame (tests/inter_residual_cases.py) -- the committed fixture against a fresh
composition from the compiled reference and from the oracle, what the fixture must contain, the coefficient layout against
xy_to_zorder, and the composed coded-block flags through the deblocking filter of both backends."""
import os

import numpy as np
import pytest

import inter_recon_cases as IC
import inter_residual_cases as RC
import oracle_lib as O
import ref_lib as R
from patterns import deblock_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_residual.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")


def _check_fixture(B):
    z = np.load(GOLDEN, allow_pickle=False)
    fresh, missing = RC.build_fixture(B)
    assert not missing
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)


@needs_ref
def test_fixture_regenerates_from_the_compiled_reference():
    _check_fixture(R)


def test_fixture_regenerates_from_the_oracle():
    _check_fixture(O)


def test_fixture_is_small_numeric_and_covers_every_tu_kind():
    assert os.path.getsize(GOLDEN) < 600 * 1024
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "ui" for k in z.files)
    pics = RC.FIXTURE_PICTURES
    assert len({p[4] for p in pics}) >= 3 and any(p[5] for p in pics) and any(not p[3] for p in pics) and any(p[2] % 64 for p in pics if p[3])
    assert "mono_rec_u" not in z.files and z["ragged_rec_y"].shape == (136, 200)
    tus, maps = [], []
    for (name, w, h, chroma, qp, signhide, seed) in pics:
        tus += [tuple(int(v) for v in t) for t in z[name + "_tus"]]
        maps.append((RC.load_fixture_case(z, name, chroma)[2], w, h))
    assert RC.coverage(tus, maps) == []


def test_coefficient_layout_is_xy_to_zorder():
    """a direct restatement of cu.h:373-410 for every TU position of an LCU: the offsets of the composition, and that TUs tile the
    LCU's array without overlap at every size"""
    def direct(width, x, y):
        r = 0
        if width == 64:
            r += x // 32 * (32 * 32) + y // 32 * (64 * 32); x %= 32; y %= 32
        r += x // 16 * (16 * 16) + y // 16 * (32 * 16); x %= 16; y %= 16
        r += x // 8 * (8 * 8) + y // 8 * (16 * 8); x %= 8; y %= 8
        r += x // 4 * (4 * 4) + y // 4 * (8 * 4)
        return r
    for width in (64, 32):
        for n in (4, 8, 16, 32):
            used = np.zeros(width * width, dtype=np.int32)
            for y in range(0, width, n):
                for x in range(0, width, n):
                    z = RC.xy_to_zorder(width, x, y)
                    assert z == direct(width, x, y)
                    used[z:z + n * n] += 1
            assert (used == 1).all()
    # one TU in an otherwise empty picture lands where the layout says
    cus = np.zeros((32, 32), dtype=RC.CU_INFO)
    blk = cus[20:24, 8:12]
    blk["type"], blk["depth"], blk["tr_depth"], blk["mv_dir"] = IC.CU_INTER, 2, 2, 1
    pred = RC.smooth_planes(128, 128, 1)
    src = tuple(np.clip(p.astype(int) + 30 * ((np.indices(p.shape).sum(axis=0) % 3) - 1), 0, 255).astype(np.uint8) for p in pred)
    out = RC.compose(src, pred, cus, 22, B=O)
    lcu = 1 * 2 + 0
    for k in range(3):
        nz = np.nonzero(out["coeff"][k].reshape(-1))[0]
        n, per, lw = (16, 4096, 64) if k == 0 else (8, 1024, 32)
        z0 = lcu * per + direct(lw, (32 % 64) >> (k > 0), (80 % 64) >> (k > 0))
        assert len(nz) and nz.min() >= z0 and nz.max() < z0 + n * n


def test_walk_follows_tr_depth_from_the_map():
    cus, _ = RC.make_map(256, 192, 5, n_refs=2)
    tus = RC.walk_tus(cus, 256, 192)
    luma = np.zeros((192, 256), np.int32)
    for (p, x, y, n, cx, cy) in tus:
        if p == 0:
            luma[y:y + n, x:x + n] += 1
            d = int(cus[cy // 4, cx // 4]["depth"])
            assert n == 64 >> min(4, max(d, int(cus[y // 4, x // 4]["tr_depth"]), 1))
    m = np.zeros((192, 256), bool)
    deeper = 0
    for (x, y, s) in RC.inter_cus(cus, 256, 192):
        m[y:y + s, x:x + s] = True
        d = {64: 0, 32: 1, 16: 2, 8: 3}[s]
        deeper += int(cus[y // 4, x // 4]["tr_depth"]) > (max(1, d) if cus[y // 4, x // 4]["part_size"] == 0 else d + 1)
    assert deeper > 5 and (luma[m] == 1).all() and (luma[~m] == 0).all()
    # chroma: every 8x8 luma area of an inter CU is covered once per plane
    for p in (1, 2):
        c = np.zeros((96, 128), np.int32)
        for (q, x, y, n, _, _) in tus:
            if q == p:
                c[y // 2:y // 2 + n, x // 2:x // 2 + n] += 1
        assert (c[m[::2, ::2]] == 1).all() and (c[~m[::2, ::2]] == 0).all()


def test_numpy_sums_equal_the_reference_functions():
    name, w, h, chroma, qp, signhide, seed = RC.FIXTURE_PICTURES[0]
    src, pred, cus = RC.fixture_case(name, w, h, chroma, qp, signhide, seed)
    init = RC.initial_outputs(w, h, chroma)
    RC.assert_outputs_equal(RC.compose(src, pred, cus, qp, chroma, signhide, B=O, init=init, many=True),
                            RC.compose(src, pred, cus, qp, chroma, signhide, B=RC.backend(), init=init), "many vs per TU")


@pytest.mark.parametrize("pic", RC.FIXTURE_PICTURES, ids=[p[0] for p in RC.FIXTURE_PICTURES])
def test_composed_flags_deblock_alike_in_reference_and_oracle(pic):
    """the chain residual coding -> deblocking: the composed reconstruction and cbf_y through both deblocking filters"""
    name, w, h, chroma, qp, signhide, seed = pic
    z = np.load(GOLDEN, allow_pickle=False)
    _, _, _, want = RC.load_fixture_case(z, name, chroma)
    prm = deblock_params(qp=qp, chroma=chroma)
    y, u, v = want["rec"]
    a = O.deblock_frame(y, u, v, want["cus"], prm)
    assert not np.array_equal(a[0], y)
    if R.available():
        b = R.deblock_frame(y, u, v, want["cus"], prm)
        for k in range(3 if chroma else 1):
            np.testing.assert_array_equal(a[k], b[k])

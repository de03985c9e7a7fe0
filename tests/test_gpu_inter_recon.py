"""GPU: kvz_hip_inter_recon_batch / kvz_hip_inter_recon_frame against the prediction composed from the reference's own functions
(tests/inter_recon_cases.py: the compiled reference where it was built, else the oracle pinned to it), against the committed
fixture, and -- at 1920x1080 -- against the chain of existing entries over every pixel.  Every destination starts poisoned and every
comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import inter_recon_cases as IC
from patterns import CU_INFO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_recon.npz")
POISON = 0x5A


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


def poisoned(w, h, chroma=1, pad=0):
    """destination planes full of poison, `pad` extra columns (a stride beyond the width)"""
    return tuple(np.full((h >> (1 if k else 0), (w >> (1 if k else 0)) + pad), POISON, np.uint8) if (k == 0 or chroma) else None for k in range(3))


def assert_planes_equal(got, want, what=""):
    for k, n in enumerate("yuv"):
        if want[k] is None:
            assert got[k] is None
            continue
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s plane %s" % (what, n))


def pack_cells(items, w, h, cell, g):
    """PUs (shape, mv_dir, mv0, mv1, ref0, ref1) placed one per cell x cell square of the picture (a random 4-aligned offset inside it),
    cut into lists that fit one picture: PUs of one call never overlap"""
    per = (w // cell) * (h // cell)
    calls = []
    for lo in range(0, len(items), per):
        pus = []
        for i, ((pw, ph), d, mv0, mv1, r0, r1) in enumerate(items[lo:lo + per]):
            cx, cy = (i % (w // cell)) * cell, (i // (w // cell)) * cell
            ox, oy = 4 * int(g.integers(0, (cell - pw) // 4 + 1)), 4 * int(g.integers(0, (cell - ph) // 4 + 1))
            pus.append(IC.make_pu(cx + ox, cy + oy, pw, ph, d, mv0, mv1, r0, r1))
        calls.append(np.array(pus, dtype=IC.INTER_PU))
    return calls


def run_batch_cases(api, items, w, h, cell, seed, n_refs=3):
    g = np.random.default_rng(seed)
    refs = IC.random_planes(w, h, seed, n_refs, pad=(20, 2))          # strides beyond the width, the padding poisoned
    for n, pus in enumerate(pack_cells(items, w, h, cell, g)):
        dest = poisoned(w, h, pad=12)
        want = IC.compose(refs, pus, (h, w), 1, tuple(d[:, :d.shape[1] - 12] for d in dest))
        got = api.inter_recon_batch(refs, pus, (h, w), 1, dest)
        for k in range(3):
            assert (got[k][:, -12:] == POISON).all(), "wrote beyond the width"
        assert_planes_equal(tuple(p[:, :-12] for p in got), want, "call %d" % n)


def test_batch_every_shape_and_direction(api):
    g = np.random.default_rng(1)
    items = []
    for shape in IC.PU_SHAPES:
        for d in (1, 2, 3):
            for _ in range(4):
                items.append((shape, d, IC.random_mv(g, 256, 192, 0.2), IC.random_mv(g, 256, 192, 0.2), int(g.integers(0, 3)), int(g.integers(0, 3))))
    run_batch_cases(api, items, 256, 192, 64, 11)


def test_batch_all_64_fraction_pairs(api):
    """(mv_x & 7, mv_y & 7): all 16 luma and 64 chroma fractions and the luma-integer / chroma-fractional mix, on the other list a random vector"""
    g = np.random.default_rng(2)
    items = []
    shapes = ((8, 8), (4, 8), (8, 4), (16, 16), (12, 16), (16, 4), (32, 24), (32, 32))
    for fx in range(8):
        for fy in range(8):
            for d in (1, 2, 3):
                for shape in (shapes[(fx + 3 * fy + d) % 8], shapes[(fx + 3 * fy + d + 4) % 8]):
                    base = (8 * int(g.integers(-6, 7)), 8 * int(g.integers(-6, 7)))
                    mv = (base[0] + fx, base[1] + fy)
                    other = IC.random_mv(g, 256, 192, 0.0)
                    items.append((shape, d, mv if d != 2 else other, mv if d == 2 else other, int(g.integers(0, 3)), int(g.integers(0, 3))))
    run_batch_cases(api, items, 256, 192, 32, 12)


def test_batch_vectors_beyond_the_picture(api):
    """windows partly and wholly outside on every side and corner: vectors up to +-(picture size + 80) pixels"""
    g = np.random.default_rng(3)
    w, h = 128, 128
    items = []
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for shape in ((8, 8), (16, 16), (4, 16), (64, 64), (24, 32), (64, 16)):
                for d in (1, 3):
                    # near the edge (partly outside) and far (wholly outside)
                    for reach in (0, 1):
                        mvx = 4 * sx * ((w - 8 if reach == 0 else w + 80) - int(g.integers(0, 12))) + int(g.integers(0, 8))
                        mvy = 4 * sy * ((h - 8 if reach == 0 else h + 80) - int(g.integers(0, 12))) + int(g.integers(0, 8))
                        items.append((shape, d, (mvx, mvy), IC.random_mv(g, w, h, 0.5), 0, 1))
    run_batch_cases(api, items, w, h, 64, 13, n_refs=2)


MAPS = [(128, 64, 1, False, 1), (200, 136, 2, False, 1), (136, 72, 3, True, 1), (256, 192, 4, True, 1), (96, 72, 2, True, 0)]


@pytest.mark.parametrize("w,h,n_refs,slice_b,chroma", MAPS)
def test_frame_equals_reference_and_batch(api, w, h, n_refs, slice_b, chroma):
    refs = IC.random_planes(w, h, 40 + w, n_refs, pad=(8, 1), chroma=chroma)
    cus, ref_LX = IC.random_cu_map(w, h, 50 + w, n_refs, slice_b)
    pus = IC.walk_pus(cus, ref_LX, w, h)
    assert len(pus) > 4
    want = IC.compose(refs, pus, (h, w), chroma, poisoned(w, h, chroma))
    got = api.inter_recon_frame(refs, cus, ref_LX, w, h, chroma, poisoned(w, h, chroma))        # 4:0:0: NULL U / V
    assert_planes_equal(got, want, "frame vs reference")
    assert_planes_equal(api.inter_recon_batch(refs, pus, (h, w), chroma, poisoned(w, h, chroma)), got, "batch vs frame")
    # every destination pixel outside an inter PU still holds the poison
    m = IC.inter_mask(pus, (h, w), n_refs)
    assert m.any() and not m.all()
    assert (got[0][~m] == POISON).all()
    if chroma:
        mc = m[::2, ::2]
        assert (got[1][~mc] == POISON).all() and (got[2][~mc] == POISON).all()


def test_frame_equals_the_committed_fixture(api):
    z = np.load(GOLDEN, allow_pickle=False)
    for (name, w, h, n_refs, slice_b, chroma, seed) in IC.FIXTURE_PICTURES:
        refs, cus, ref_LX, pus, want = IC.load_fixture_case(z, name, n_refs, chroma)
        got = api.inter_recon_frame(refs, cus, ref_LX, w, h, chroma, poisoned(w, h, chroma))
        assert_planes_equal(got, want, name)
        assert_planes_equal(api.inter_recon_batch(refs, pus, (h, w), chroma, poisoned(w, h, chroma)), want, name + " batch")


def chain_prediction(api, refs, pus, w, h):
    """the same planes from the entries that existed before: sample_*_batch (8-bit for uni-prediction, 14-bit + bipred_blend_batch for
    bi-prediction) and clamped copies for integer planes"""
    out = poisoned(w, h)
    valid = [p for p in pus if IC.pu_valid(p, w, h, len(refs))]
    for k in range(3):                                   # plane
        c = 1 if k else 0
        kind, fm, ish = ("chroma", 7, 3) if k else ("luma", 3, 2)
        src = {}                                         # (pu index, list) -> block (int16 14-bit, or uint8)
        jobs = {}                                        # (picture, 14-bit) -> [(pu index, list, block descriptor)]
        for i, p in enumerate(valid):
            d = int(p["mv_dir"])
            for lst in range(2):
                if not d & (1 << lst):
                    continue
                mvx, mvy = int(p["mv"][lst][0]), int(p["mv"][lst][1])
                x, y, pw, ph = (int(p["x"]) >> c) + (mvx >> ish), (int(p["y"]) >> c) + (mvy >> ish), int(p["width"]) >> c, int(p["height"]) >> c
                if (mvx & fm) or (mvy & fm):
                    jobs.setdefault((int(p["ref"][lst]), d == 3), []).append((i, lst, (x, y, mvx & fm, mvy & fm, pw, ph)))
                else:
                    src[(i, lst)] = IC.gather(refs[int(p["ref"][lst])][k][:h >> c, :w >> c], x, y, pw, ph)
        for (pic, hi), lst_jobs in jobs.items():
            blocks = api.sample_batch(kind + ("14" if hi else ""), refs[pic][k], [j[2] for j in lst_jobs], ref_w=w >> c, ref_h=h >> c)
            for (i, lst, _), b in zip(lst_jobs, blocks):
                src[(i, lst)] = b
        blends = {}                                      # (w, h, hi0, hi1) -> [pu index]
        for i, p in enumerate(valid):
            x, y, pw, ph = int(p["x"]) >> c, int(p["y"]) >> c, int(p["width"]) >> c, int(p["height"]) >> c
            if int(p["mv_dir"]) != 3:
                out[k][y:y + ph, x:x + pw] = src[(i, int(p["mv_dir"]) - 1)]
            else:
                blends.setdefault((pw, ph, src[(i, 0)].dtype == np.int16, src[(i, 1)].dtype == np.int16), []).append(i)
        for (pw, ph, hi0, hi1), idx in blends.items():
            res = api.bipred_blend_batch(pw, ph, hi0, np.stack([src[(i, 0)] for i in idx]), hi1, np.stack([src[(i, 1)] for i in idx]))
            for i, b in zip(idx, res):
                x, y = int(valid[i]["x"]) >> c, int(valid[i]["y"]) >> c
                out[k][y:y + ph, x:x + pw] = b
    return out


@pytest.mark.parametrize("slice_b", [False, True])
def test_full_hd_frame_equals_the_chain_and_the_reference(api, slice_b):
    w, h, n_refs = 1920, 1080, 2 if slice_b else 1
    refs = IC.random_planes(w, h, 70, n_refs)
    cus, ref_LX = IC.random_cu_map(w, h, 71 + slice_b, n_refs, slice_b, far=0.01)
    pus = IC.walk_pus(cus, ref_LX, w, h)
    got = api.inter_recon_frame(refs, cus, ref_LX, w, h, 1, poisoned(w, h))
    assert_planes_equal(got, chain_prediction(api, refs, pus, w, h), "frame vs chain")
    assert_planes_equal(got, IC.compose(refs, pus, (h, w), 1, poisoned(w, h)), "frame vs reference")


def test_zero_vectors_give_the_reference_picture(api):
    w, h = 192, 128
    refs = IC.random_planes(w, h, 80, 1)
    cus, ref_LX = IC.random_cu_map(w, h, 81, 1, False, bad_share=0.0)
    cus["mv"] = 0
    got = api.inter_recon_frame(refs, cus, ref_LX, w, h, 1, poisoned(w, h))
    m = IC.inter_mask(IC.walk_pus(cus, ref_LX, w, h), (h, w), 1)
    for k in range(3):
        mk = m[::2, ::2] if k else m
        np.testing.assert_array_equal(got[k][mk], refs[0][k][mk])
        assert (got[k][~mk] == POISON).all()


def test_result_does_not_depend_on_order_or_on_how_the_list_is_cut(api):
    w, h = 256, 192
    refs = IC.random_planes(w, h, 90, 3)
    cus, ref_LX = IC.random_cu_map(w, h, 91, 3, True)
    pus = IC.walk_pus(cus, ref_LX, w, h)
    whole = api.inter_recon_batch(refs, pus, (h, w), 1, poisoned(w, h))
    g = np.random.default_rng(92)
    shuffled = pus[g.permutation(len(pus))]
    assert_planes_equal(api.inter_recon_batch(refs, shuffled, (h, w), 1, poisoned(w, h)), whole, "shuffled")
    dest = poisoned(w, h)
    cuts = [0, 1, 2, 7, len(pus) // 3, len(pus) // 3 + 5, len(pus)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        dest = api.inter_recon_batch(refs, shuffled[lo:hi], (h, w), 1, dest)
    assert_planes_equal(dest, whole, "in pieces")


def test_bad_descriptors_write_nothing(api):
    w, h = 128, 96
    refs = IC.random_planes(w, h, 95, 2)
    good = [IC.make_pu(0, 0, 16, 16, 1, (5, 3)), IC.make_pu(64, 32, 32, 32, 3, (-9, 2), (4, 4), 0, 1), IC.make_pu(96, 64, 8, 4, 2, (0, 0), (1, 1), 0, 1)]
    bad = [IC.make_pu(16, 0, 4, 4, 1), IC.make_pu(32, 0, 12, 12, 1), IC.make_pu(16, 16, 10, 8, 1), IC.make_pu(16, 32, 72, 8, 1), IC.make_pu(32, 32, 0, 8, 1),
           IC.make_pu(120, 0, 16, 16, 1), IC.make_pu(0, 88, 16, 16, 1), IC.make_pu(-4, 16, 8, 8, 1), IC.make_pu(18, 48, 8, 8, 1), IC.make_pu(32, 50, 8, 8, 1),
           IC.make_pu(48, 0, 8, 8, 0), IC.make_pu(48, 8, 8, 8, 4), IC.make_pu(48, 16, 8, 8, 1, ref0=2), IC.make_pu(48, 24, 8, 8, 2, ref1=200),
           IC.make_pu(48, 32, 8, 8, 3, ref0=0, ref1=2), IC.make_pu(56, 0, -8, 8, 1)]
    mixed = np.array([bad[0], good[0]] + bad[1:9] + [good[1]] + bad[9:] + [good[2]], dtype=IC.INTER_PU)
    want = IC.compose(refs, np.array(good, dtype=IC.INTER_PU), (h, w), 1, poisoned(w, h))
    assert_planes_equal(api.inter_recon_batch(refs, mixed, (h, w), 1, poisoned(w, h)), want, "good among bad")
    only_bad = api.inter_recon_batch(refs, np.array(bad, dtype=IC.INTER_PU), (h, w), 1, poisoned(w, h))
    assert all((p == POISON).all() for p in only_bad)


def test_count_zero_and_bad_arguments(api):
    from kvazaar_amd import _lib
    L = _lib.init(0)
    w, h = 64, 64
    refs = IC.random_planes(w, h, 96, 1)
    got = api.inter_recon_batch(refs, np.zeros(0, dtype=IC.INTER_PU), (h, w), 1, poisoned(w, h))
    assert all((p == POISON).all() for p in got)
    st = api._Recon(refs, (h, w), 1, poisoned(w, h))
    pus = api.DeviceBuffer.from_numpy(np.array([IC.make_pu(0, 0, 8, 8, 1)], dtype=IC.INTER_PU).view(np.uint8))
    cus = api.DeviceBuffer.from_numpy(np.zeros((16, 16), dtype=CU_INFO).view(np.uint8))
    prm = np.zeros(1, dtype=api.INTER_RECON_PARAMS)
    prm["chroma"], prm["n_refs"] = 1, 1
    t = st.table.ctypes.data

    def batch(table=t, n=1, p=pus.ptr, count=1, y=st.dptr(0), u=st.dptr(1), v=st.dptr(2), chroma=1):
        return L.kvz_hip_inter_recon_batch(table, n, p, count, y, w, u, v, w // 2, chroma, None)

    def frame(y=st.dptr(0), u=st.dptr(1), c=cus.ptr, table=t, p=prm.ctypes.data, width=w):
        return L.kvz_hip_inter_recon_frame(y, w, u, st.dptr(2), w // 2, width, h, c, table, p, None)
    assert batch() == 0 and frame() == 0
    assert batch(count=0) == 0 and batch(p=None, count=0) == 0
    assert batch(u=None, v=None, chroma=0) == 0                              # 4:0:0: U / V unused
    for rc in (batch(table=None), batch(n=0), batch(n=17), batch(p=None), batch(y=None), batch(u=None), batch(v=None)):
        assert rc == -2 and b"kvz_hip_inter_recon_batch" in L.kvz_hip_last_error()
    for rc in (frame(y=None), frame(u=None), frame(c=None), frame(table=None), frame(p=None), frame(width=60)):
        assert rc == -2 and b"kvz_hip_inter_recon_frame" in L.kvz_hip_last_error()
    assert L.kvz_hip_abi_version() == 4


def test_frame_graph_replay_follows_the_cu_array(api):
    """the frame entry captured once (kvz_hip_graph_begin / _end) and replayed after the CU array's contents were replaced"""
    from kvazaar_amd import _lib
    L = _lib.init(0)
    w, h, n_refs = 200, 136, 3
    refs = IC.random_planes(w, h, 97, n_refs)
    maps = [IC.random_cu_map(w, h, 98 + i, n_refs, True) for i in range(3)]
    ref_LX = maps[0][1]
    st = api._Recon(refs, (h, w), 1, poisoned(w, h))
    prm = np.zeros(1, dtype=api.INTER_RECON_PARAMS)
    prm["chroma"], prm["n_refs"], prm["ref_LX"] = 1, n_refs, ref_LX
    d_cus = api.DeviceBuffer.from_numpy(maps[0][0].view(np.uint8))
    s = L.kvz_hip_stream_create()
    graph = C.c_void_p()
    _lib.check(L.kvz_hip_graph_begin(s), "graph_begin")
    _lib.check(L.kvz_hip_inter_recon_frame(st.dptr(0), w, st.dptr(1), st.dptr(2), w // 2, w, h, d_cus.ptr, st.table.ctypes.data, prm.ctypes.data, s), "frame")
    _lib.check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
    assert graph.value
    try:
        for cus, _ in maps[1:] + maps[:1]:
            cus = np.ascontiguousarray(cus)
            for b, p in zip(st.dbuf, poisoned(w, h)):
                _lib.check(L.kvz_hip_memcpy_h2d(b.ptr, p.ctypes.data, p.nbytes, s), "h2d")
            _lib.check(L.kvz_hip_memcpy_h2d(d_cus.ptr, cus.ctypes.data, cus.nbytes, s), "h2d")
            _lib.check(L.kvz_hip_stream_sync(s), "sync")
            _lib.check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            _lib.check(L.kvz_hip_stream_sync(s), "sync")
            got = st.result()
            eager = api.inter_recon_frame(refs, cus, ref_LX, w, h, 1, poisoned(w, h))
            assert_planes_equal(got, eager, "replay vs eager")
            assert_planes_equal(got, IC.compose(refs, IC.walk_pus(cus, ref_LX, w, h), (h, w), 1, poisoned(w, h)), "replay vs reference")
    finally:
        L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)

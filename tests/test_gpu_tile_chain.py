"""GPU: the four tile entries of the picture chain -- kvz_hip_intra_recon_frame_tiles, kvz_hip_cu_qp_frame_tiles,
kvz_hip_deblock_frame_tiles and kvz_hip_sao_frame_tiles -- against the committed fixture and the composition of the reference's own
functions tile by tile (tests/tile_chain_cases.py); against the untiled entries, with no grid, with a grid of one tile, and run tile by
tile on offset plane pointers; for isolation between tiles; in the chain on one stream, eager and replayed from a captured graph; and
for what they refuse.  Every output starts poisoned, every array is staged between guard bands, every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import lcu_qp_cases as QC
import oracle_lib as O
import test_gpu_inter_residual as TR
import test_gpu_lcu_qp as QL
import tile_chain_cases as TC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_chain.npz")
LCU_QP_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "lcu_qp.npz")
POISON_DST = 0x3C
INVALID = -2


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


check = QL.check


class Staged(QL.Staged):
    """the staging of the per-LCU-QP tests plus the SAO records, the SAO destination and the grid"""

    def __init__(self, A, case, init=None):
        w, h, chroma = case["width"], case["height"], case["chroma"]
        QL.Staged.__init__(self, A, case["src"], case["pred"], case["cus"], case["modes"], case["lcu_qp"], QC.PARAMS_QP, chroma, case["signhide"],
                           case["slice_is_intra"], init=init or QC.zero_outputs(w, h, chroma))
        self.host["dst"] = [np.full(p.shape, POISON_DST, np.uint8) for p in self.host["rec"]]
        self.host["sao"] = [np.ascontiguousarray(s, dtype=np.int32) for s in (case["sao_luma"], case["sao_chroma"]) if s is not None]
        for k in ("dst", "sao"):
            self.dev[k] = [self._up(a) for a in self.host[k]]
        self.grid = A.tile_grid(w, h, case["col_bd"], case["row_bd"])
        self.tprm = np.zeros(1, dtype=A.CU_QP_TILES_PARAMS)
        self.dprm = TC.chain_deblock_params(case)
        self.start_qp = case["start_qp"]

    def intra_tiles(self, stream=None, **over):
        a = self.args(over)
        return self.L.kvz_hip_intra_recon_frame_tiles(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["modes"], a["cy"], a["cu"], a["cv"],
                                                      a["cbf"], a["costs"], a.get("lcu_qp", self.qp_ptr()), a.get("grid", self.grid.ctypes.data), a["prm"],
                                                      stream)

    def cu_qp_tiles(self, chain_rows=0, stream=None, start_qp=None, **over):
        self.tprm["start_qp"], self.tprm["chain_rows"] = self.start_qp if start_qp is None else start_qp, chain_rows
        a = {"cus": self.ptr("cus"), "cbf": self.ptr("cbf_out"), "w": self.w, "h": self.h, "lcu_qp": self.qp_ptr(), "last": self.ptr("last"),
             "grid": self.grid.ctypes.data, "prm": self.tprm.ctypes.data}
        a.update(over)
        return self.L.kvz_hip_cu_qp_frame_tiles(a["cus"], a["cbf"], a["w"], a["h"], a["lcu_qp"], a["last"], a["grid"], a["prm"], stream)

    def plane_args(self, over):
        a = {"y": self.ptr("rec", 0), "sy": self.w, "u": self.ptr("rec", 1), "v": self.ptr("rec", 2), "sc": self.w // 2 if self.chroma else 0,
             "w": self.w, "h": self.h, "cus": self.ptr("cus"), "grid": self.grid.ctypes.data, "prm": self.dprm.ctypes.data,
             "dy": self.ptr("dst", 0), "du": self.ptr("dst", 1), "dv": self.ptr("dst", 2), "luma": self.ptr("sao", 0), "chro": self.ptr("sao", 1),
             "chroma": self.chroma}
        a.update(over)
        return a

    def deblock_tiles(self, stream=None, **over):
        a = self.plane_args(over)
        return self.L.kvz_hip_deblock_frame_tiles(a["y"], a["sy"], a["u"], a["v"], a["sc"], a["w"], a["h"], a["cus"], a["grid"], a["prm"], stream)

    def deblock(self, stream=None):
        a = self.plane_args({})
        return self.L.kvz_hip_deblock_frame(a["y"], a["sy"], a["u"], a["v"], a["sc"], a["w"], a["h"], a["cus"], a["prm"], stream)

    def sao_args(self, a):
        return (a["y"], a["sy"], a["u"], a["v"], a["sc"], a["dy"], a["sy"], a["du"], a["dv"], a["sc"], a["w"], a["h"], a["luma"], a["chro"], a["chroma"])

    def sao_tiles(self, stream=None, **over):
        a = self.plane_args(over)
        return self.L.kvz_hip_sao_frame_tiles(*self.sao_args(a), a["grid"], stream)

    def sao(self, stream=None):
        return self.L.kvz_hip_sao_frame(*self.sao_args(self.plane_args({})), stream)

    def chain(self, stream=None, chain_rows=0):
        check(self.inter_qp(stream), "inter_residual_frame_qp")
        check(self.intra_tiles(stream), "intra_recon_frame_tiles")
        check(self.cu_qp_tiles(chain_rows, stream), "cu_qp_frame_tiles")
        check(self.deblock_tiles(stream), "deblock_frame_tiles")
        check(self.sao_tiles(stream), "sao_frame_tiles")

    def sync(self, stream=None):
        check(self.L.kvz_hip_stream_sync(stream), "sync")

    def result(self):
        out = QL.Staged.result(self)                                   # asserts every guard band, the source, the modes and the QP array
        pad = [None] * (3 - self.n)
        out["dst"] = tuple([self.raw("dst", k)[TR.GUARD:-TR.GUARD].reshape(self.host["dst"][k].shape) for k in range(self.n)] + pad)
        for k, s in enumerate(self.host["sao"]):
            np.testing.assert_array_equal(self.raw("sao", k)[TR.GUARD:-TR.GUARD].view(np.int32).reshape(s.shape), s, err_msg="the SAO records were written")
        return out


def assert_planes(got, want, what):
    for k in range(3):
        if want[k] is not None:
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s: plane %d" % (what, k))


def assert_chain(got, want, what, chroma=1, rows=False):
    """the state after the whole chain: planes deblocked in place, the SAO destination, the map with qp, everything of the residual stages"""
    assert_planes(got["rec"], want["deb"], what + " after deblocking")
    assert_planes(got["dst"], want["sao"], what + " after SAO")
    for k in range(3 if chroma else 1):
        np.testing.assert_array_equal(got["coeff"][k], want["full"]["coeff"][k], err_msg="%s: coefficients %d" % (what, k))
    np.testing.assert_array_equal(got["cus"].view(np.uint8), want["cus_qp_rows" if rows else "cus_qp"].view(np.uint8), err_msg=what + ": the map")
    np.testing.assert_array_equal(got["last"], want["last_rows" if rows else "last"], err_msg=what + ": lcu_last_qp")
    np.testing.assert_array_equal(got["cbf_out"], want["full"]["cbf_out"], err_msg=what)
    np.testing.assert_array_equal(got["costs"].view(np.uint32), want["full"]["costs"].view(np.uint32), err_msg=what)


# ---------------------------------------------------------------- 1. the fixture, entry by entry
@pytest.mark.parametrize("pic", TC.FIXTURE_PICTURES, ids=[p[0] for p in TC.FIXTURE_PICTURES])
def test_fixture_through_the_four_entries_one_by_one(api, pic):
    case, want = TC.load_fixture_case(np.load(GOLDEN, allow_pickle=False), pic)
    name, chroma = case["name"], case["chroma"]
    wants = [(want, "fixture")]
    if name == "ragged":
        wants.append((TC.compose_chain(case, O), "oracle"))
    st = Staged(api, case)
    check(st.inter_qp(), "inter_residual_frame_qp")
    check(st.intra_tiles(), "intra_recon_frame_tiles")
    st.sync()
    got = st.result()
    for w_, what in wants:
        QC.assert_outputs_equal(got, w_["full"], "%s intra vs %s" % (name, what), chroma)
    assert (got["last"] == QL.POISON_LAST).all() and all((d == POISON_DST).all() for d in got["dst"] if d is not None)
    for rows in (1, 0):
        st.upload("cus", 0, want["full"]["cus"])
        check(st.cu_qp_tiles(rows), "cu_qp_frame_tiles")
        st.sync()
        got = st.result()
        for w_, what in wants:
            np.testing.assert_array_equal(got["cus"].view(np.uint8), w_["cus_qp_rows" if rows else "cus_qp"].view(np.uint8), err_msg="%s chain_rows %d" % (what, rows))
            np.testing.assert_array_equal(got["last"], w_["last_rows" if rows else "last"], err_msg="%s chain_rows %d" % (what, rows))
    check(st.deblock_tiles(), "deblock_frame_tiles")
    st.sync()
    got = st.result()
    for w_, what in wants:
        assert_planes(got["rec"], w_["deb"], "%s deblocking vs %s" % (name, what))
    np.testing.assert_array_equal(got["cus"].view(np.uint8), want["cus_qp"].view(np.uint8), err_msg="deblocking wrote the map")
    check(st.sao_tiles(), "sao_frame_tiles")
    st.sync()
    got = st.result()
    for w_, what in wants:
        assert_chain(got, w_, "%s vs %s" % (name, what), chroma)


# ---------------------------------------------------------------- 2. no grid and one tile are the untiled entries
def test_null_grid_and_one_tile_are_the_untiled_entries_byte_for_byte(api):
    z = np.load(LCU_QP_GOLDEN, allow_pickle=False)
    pic = QC.FIXTURE_PICTURES[0]
    name, w, h, chroma, signhide, slice_is_intra, seed, share, start_qp, _ = pic
    assert (name, w, h) == ("ragged", 200, 136)
    src, pred, cus, modes, lcu_qp, _ = QC.load_fixture_case(z, name, chroma)
    luma, chro = TC.sao_records(w, h, 5, None, None)
    case = {"name": name, "width": w, "height": h, "chroma": chroma, "signhide": signhide, "slice_is_intra": slice_is_intra, "start_qp": start_qp,
            "col_bd": [0, 4], "row_bd": [0, 3], "src": src, "pred": pred, "cus": cus, "modes": modes, "lcu_qp": lcu_qp, "sao_luma": luma, "sao_chroma": chro}
    lx = QC.lcu_grid(w, h)[0]
    for rows, null_qp in ((0, False), (1, False), (0, True)):
        old = Staged(api, case)
        over = {"lcu_qp": None} if null_qp else {}
        check(old.inter_qp(**over), "inter_residual_frame_qp")
        check(old.intra_qp(**over), "intra_recon_frame_qp")
        check(old.cu_qp(start_qp, lx if rows else 0), "cu_qp_frame")
        check(old.deblock(), "deblock_frame")
        check(old.sao(), "sao_frame")
        old.sync()
        want = old.result()
        assert (want["dst"][0] != POISON_DST).any() and not np.array_equal(want["dst"][0], want["rec"][0]) and (want["last"] != QL.POISON_LAST).all()
        for grid in ("null", "one"):
            g = {"grid": None} if grid == "null" else {}
            new = Staged(api, case)
            check(new.inter_qp(**over), "inter_residual_frame_qp")
            check(new.intra_tiles(**over, **g), "intra_recon_frame_tiles")
            check(new.cu_qp_tiles(rows, **g), "cu_qp_frame_tiles")
            check(new.deblock_tiles(**g), "deblock_frame_tiles")
            check(new.sao_tiles(**g), "sao_frame_tiles")
            new.sync()
            got = new.result()
            what = "grid %s, chain_rows %d, lcu_qp %s" % (grid, rows, "NULL" if null_qp else "given")
            QC.assert_outputs_equal({k: got[k] for k in ("rec", "coeff", "cus", "cbf_out", "costs")}, want, what, chroma)
            assert_planes(got["dst"], want["dst"], what + " SAO")
            np.testing.assert_array_equal(got["last"], want["last"], err_msg=what)


# ---------------------------------------------------------------- 3. against the untiled entries run tile by tile, without the CPU
DIFF_PIC = ("diff", 448, 264, 1, 1, 0, 4400, 0.5, 29, (0, 2, 3, 7), (0, 1, 5))
# more tile columns than the kernels' lookups take in their first part (tile_grid.h: TILE_NEAR = 8): every LCU a tile, ragged bottom
MANY_PIC = ("many", 640, 72, 1, 0, 0, 4700, 0.5, 31, tuple(range(11)), (0, 1, 2))


class DevArray:
    def __init__(self, A, a):
        self.a = np.ascontiguousarray(a)
        self.buf = A.DeviceBuffer.from_numpy(self.a.view(np.uint8).reshape(-1))
        self.ptr = self.buf.ptr

    def get(self):
        return self.buf.to_numpy(np.uint8, (self.a.nbytes,)).view(self.a.dtype).reshape(self.a.shape)


def chain_tile_by_tile(A, L, case, chain_rows):
    """intra -> QP map -> deblocking -> SAO with the UNTILED entries, one tile at a time: plane pointers offset to the tile, compact copies
    of the tile's map, modes, cbf bytes, costs and per-LCU arrays.  -> the picture-wide results, stitched by the test"""
    w, h, chroma = case["width"], case["height"], case["chroma"]
    n = 3 if chroma else 1
    src = [DevArray(A, p) for p in case["src"][:n]]
    rec = [DevArray(A, p) for p in case["pred"][:n]]
    dst = [DevArray(A, np.full(p.shape, POISON_DST, np.uint8)) for p in case["pred"][:n]]
    zero = QC.zero_outputs(w, h, chroma)
    out = {"coeff": [np.array(c) for c in zero[0][:n]], "cus": np.array(case["cus"]), "cbf_out": np.array(zero[1]), "costs": np.array(zero[2]),
           "last": np.zeros(len(case["lcu_qp"]), np.int8)}
    prm = A.inter_residual_params(QC.PARAMS_QP, case["slice_is_intra"], case["signhide"], chroma)
    cprm, dprm = np.zeros(1, dtype=A.CU_QP_PARAMS), TC.chain_deblock_params(case)
    for t in TC.tiles(w, h, case["col_bd"], case["row_bd"]):
        x0, y0, x1, y1, lcus = t
        tw, th = x1 - x0, y1 - y0
        off = [(y0 >> (k > 0)) * (w >> (k > 0)) + (x0 >> (k > 0)) for k in range(3)]
        table = A.ref_picture_table([(src[0].ptr + off[0], src[1].ptr + off[1], src[2].ptr + off[2], w, w // 2)], tw, th)
        cus, modes = DevArray(A, TC.crop_map(case["cus"], t)), DevArray(A, TC.crop_map(case["modes"], t))
        cbf, costs = DevArray(A, TC.crop_map(zero[1], t)), DevArray(A, TC.crop_map(zero[2], t))
        coeff = [DevArray(A, zero[0][k][lcus]) for k in range(n)]
        qp, last = DevArray(A, np.asarray(case["lcu_qp"], np.int8)[lcus]), DevArray(A, np.zeros(len(lcus), np.int8))
        sl, sc = DevArray(A, case["sao_luma"][lcus]), DevArray(A, case["sao_chroma"][lcus])
        planes = (rec[0].ptr + off[0], w, rec[1].ptr + off[1], rec[2].ptr + off[2], w // 2)
        check(L.kvz_hip_intra_recon_frame_qp(table.ctypes.data, *planes, cus.ptr, modes.ptr, coeff[0].ptr, coeff[1].ptr, coeff[2].ptr, cbf.ptr, costs.ptr,
                                             qp.ptr, prm.ctypes.data, None), "intra_recon_frame_qp")
        cprm["start_qp"], cprm["chain_lcus"] = case["start_qp"], ((tw + 63) // 64 if chain_rows else 0)
        check(L.kvz_hip_cu_qp_frame(cus.ptr, cbf.ptr, tw, th, qp.ptr, last.ptr, cprm.ctypes.data, None), "cu_qp_frame")
        check(L.kvz_hip_deblock_frame(*planes, tw, th, cus.ptr, dprm.ctypes.data, None), "deblock_frame")
        check(L.kvz_hip_sao_frame(*planes, dst[0].ptr + off[0], w, dst[1].ptr + off[1], dst[2].ptr + off[2], w // 2, tw, th, sl.ptr, sc.ptr, chroma, None),
              "sao_frame")
        check(L.kvz_hip_stream_sync(None), "sync")
        blk = (slice(y0 // 4, y1 // 4), slice(x0 // 4, x1 // 4))
        out["cus"][blk], out["cbf_out"][blk], out["costs"][blk] = cus.get(), cbf.get(), costs.get()
        out["last"][lcus] = last.get()
        for k in range(n):
            out["coeff"][k][lcus] = coeff[k].get()
    out["rec"], out["dst"] = tuple(p.get() for p in rec), tuple(p.get() for p in dst)
    return out


def diff_case(pic=DIFF_PIC):
    case = TC.fixture_case(*pic)
    case["pred"] = tuple(case["pred"])
    return case


def run_tiles(api, case, chain_rows=0, inter=False):
    st = Staged(api, case)
    if inter:
        check(st.inter_qp(), "inter_residual_frame_qp")
    check(st.intra_tiles(), "intra_recon_frame_tiles")
    check(st.cu_qp_tiles(chain_rows), "cu_qp_frame_tiles")
    check(st.deblock_tiles(), "deblock_frame_tiles")
    check(st.sao_tiles(), "sao_frame_tiles")
    st.sync()
    return st.result()


@pytest.mark.parametrize("pic,chain_rows", [(DIFF_PIC, 0), (DIFF_PIC, 1), (MANY_PIC, 0)], ids=["diff-tiles", "diff-rows", "many-tiles"])
def test_tiles_entries_equal_the_untiled_entries_run_tile_by_tile(api, pic, chain_rows):
    from kvazaar_amd import _lib
    case = diff_case(pic)
    assert QC.lcu_grid(case["width"], case["height"]) == {"diff": (7, 5), "many": (10, 2)}[pic[0]] and case["height"] % 64
    got = run_tiles(api, case, chain_rows)
    want = chain_tile_by_tile(api, _lib.init(0), case, chain_rows)
    for k in range(3):
        np.testing.assert_array_equal(got["rec"][k], want["rec"][k], err_msg="plane %d after deblocking" % k)
        np.testing.assert_array_equal(got["dst"][k], want["dst"][k], err_msg="plane %d after SAO" % k)
        np.testing.assert_array_equal(got["coeff"][k], want["coeff"][k], err_msg="coefficients %d" % k)
    np.testing.assert_array_equal(got["cus"].view(np.uint8), want["cus"].view(np.uint8))
    np.testing.assert_array_equal(got["cbf_out"], want["cbf_out"])
    np.testing.assert_array_equal(got["costs"].view(np.uint32), want["costs"].view(np.uint32))
    np.testing.assert_array_equal(got["last"], want["last"])
    # the picture is no trivial one: the untiled chain gives another at every stage
    one = dict(case)
    one["col_bd"], one["row_bd"] = TC.one_tile(case["width"], case["height"])
    other = run_tiles(api, one, chain_rows)
    assert not np.array_equal(other["rec"][0], got["rec"][0]) and not np.array_equal(other["dst"][1], got["dst"][1])
    assert not np.array_equal(other["coeff"][0], got["coeff"][0])
    assert pic is not DIFF_PIC or not np.array_equal(other["last"], got["last"])


# ---------------------------------------------------------------- 4. a tile sees nothing of another
def test_changes_inside_one_tile_leave_every_other_tile_untouched(api):
    case = diff_case()
    w, h = case["width"], case["height"]
    other = TC.fixture_case(*(DIFF_PIC[:6] + (4500,) + DIFF_PIC[7:]))
    tiles = TC.tiles(w, h, case["col_bd"], case["row_bd"])
    t = tiles[4]                                                            # the middle tile of the second tile row: neighbours on every side
    x0, y0, x1, y1, lcus = t
    assert (x0, y0, x1, y1) == (128, 64, 192, 264)
    changed = dict(case)
    for key in ("src", "pred"):
        planes = [np.array(p) for p in case[key]]
        for k in range(3):
            s = 1 if k else 0
            planes[k][y0 >> s:y1 >> s, x0 >> s:x1 >> s] = other[key][k][y0 >> s:y1 >> s, x0 >> s:x1 >> s]
        changed[key] = tuple(planes)
    for key in ("cus", "modes"):
        a = np.array(case[key])
        a[y0 // 4:y1 // 4, x0 // 4:x1 // 4] = other[key][y0 // 4:y1 // 4, x0 // 4:x1 // 4]
        changed[key] = a
    a, b = run_tiles(api, case, inter=True), run_tiles(api, changed, inter=True)
    inside = np.zeros((h, w), bool)
    inside[y0:y1, x0:x1] = True
    for kind in ("rec", "dst"):
        for k in range(3):
            m = inside[::2, ::2] if k else inside
            np.testing.assert_array_equal(a[kind][k][~m], b[kind][k][~m], err_msg="%s plane %d outside the tile" % (kind, k))
            assert (a[kind][k][m] != b[kind][k][m]).any()
    ms = inside[::4, ::4]
    for key in ("cus", "costs"):
        np.testing.assert_array_equal(a[key].view(np.uint8).reshape(ms.shape + (-1,))[~ms], b[key].view(np.uint8).reshape(ms.shape + (-1,))[~ms], err_msg=key)
    np.testing.assert_array_equal(a["cbf_out"][~ms], b["cbf_out"][~ms])
    rest = np.setdiff1d(np.arange(35), lcus)
    for k in range(3):
        np.testing.assert_array_equal(a["coeff"][k][rest], b["coeff"][k][rest], err_msg="coefficients %d of the other tiles' LCUs" % k)
        assert not np.array_equal(a["coeff"][k][lcus], b["coeff"][k][lcus])
    np.testing.assert_array_equal(a["last"][rest], b["last"][rest])


# ---------------------------------------------------------------- 5. the chain on one stream, eager and replayed
def test_chain_on_one_stream_and_replayed_from_a_graph_after_the_contents_changed(api):
    pic = TC.FIXTURE_PICTURES[0]
    case, want = TC.load_fixture_case(np.load(GOLDEN, allow_pickle=False), pic)
    second = TC.fixture_case(*(pic[:6] + (4600,) + pic[7:]))
    second["sao_luma"], second["sao_chroma"] = second["sao_chroma"], second["sao_luma"]
    assert not np.array_equal(second["lcu_qp"], case["lcu_qp"]) and not np.array_equal(second["cus"].view(np.uint8), case["cus"].view(np.uint8))
    want2 = TC.compose_chain(second, O)
    st = Staged(api, case)
    L, s, graph = st.L, st.L.kvz_hip_stream_create(), C.c_void_p()
    try:
        st.chain(s)                                                     # five asynchronous calls, nothing between them
        st.sync(s)
        assert_chain(st.result(), want, "eager")
        check(L.kvz_hip_graph_begin(s), "graph_begin")
        st.chain(s)
        check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        zero = QC.zero_outputs(case["width"], case["height"], 1)
        for n, (c, w_) in enumerate(((second, want2), (case, want))):
            for k in range(3):
                st.upload("src", k, c["src"][k], s)
                st.upload("rec", k, c["pred"][k], s)
                st.upload("coeff", k, zero[0][k], s)
                st.upload("dst", k, st.host["dst"][k], s)
            st.upload("cus", 0, c["cus"], s)
            st.upload("modes", 0, c["modes"], s)
            st.upload("cbf_out", 0, zero[1], s)
            st.upload("costs", 0, zero[2], s)
            st.upload("last", 0, st.host["last"][0], s)
            st.upload("sao", 0, np.ascontiguousarray(c["sao_luma"], dtype=np.int32), s)
            st.upload("sao", 1, np.ascontiguousarray(c["sao_chroma"], dtype=np.int32), s)
            st.set_lcu_qp(c["lcu_qp"], s)
            st.sync(s)
            check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            st.sync(s)
            st.host["src"] = [np.ascontiguousarray(p) for p in c["src"]]
            st.host["modes"] = [np.ascontiguousarray(c["modes"])]
            st.host["sao"] = [np.ascontiguousarray(c["sao_luma"], dtype=np.int32), np.ascontiguousarray(c["sao_chroma"], dtype=np.int32)]
            assert_chain(st.result(), w_, "replay %d" % n)
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


# ---------------------------------------------------------------- 6. what the entries refuse
def bad_grids(A, w, h):
    lx, ly = QC.lcu_grid(w, h)
    out = []
    for edit in ("cols 0", "cols 48", "rows 0", "rows -1", "rows 48", "col_bd[0]", "row_bd[0]", "equal", "decreasing", "last col", "last row", "last col beyond"):
        g = A.tile_grid(w, h, [0, 1, lx], [0, 2, ly])
        if edit.startswith("cols") or edit.startswith("rows"):
            g[edit.split()[0]] = int(edit.split()[1])
        elif edit == "col_bd[0]":
            g["col_bd"][0, 0] = 1
        elif edit == "row_bd[0]":
            g["row_bd"][0, 0] = -1
        elif edit == "equal":
            g["row_bd"][0, 1] = 0
        elif edit == "decreasing":
            g["cols"], g["col_bd"][0, :4] = 3, (0, 2, 1, lx)
        elif edit == "last col":
            g["col_bd"][0, 2] = lx - 1
        elif edit == "last row":
            g["row_bd"][0, 2] = ly + 1
        else:
            g["col_bd"][0, 2] = lx + 1
        out.append((edit, g))
    return out


def test_refused_arguments_write_nothing(api):
    pic = TC.FIXTURE_PICTURES[0]
    case, want = TC.load_fixture_case(np.load(GOLDEN, allow_pickle=False), pic)
    w, h = case["width"], case["height"]
    init = (QC.zero_outputs(w, h, 1)[0], np.full(case["cus"].shape, 0x5D, np.uint8), QC.zero_outputs(w, h, 1)[2])
    st = Staged(api, case, init=init)
    L = st.L
    calls = {"kvz_hip_intra_recon_frame_tiles": st.intra_tiles, "kvz_hip_cu_qp_frame_tiles": lambda **o: st.cu_qp_tiles(0, **o),
             "kvz_hip_deblock_frame_tiles": st.deblock_tiles, "kvz_hip_sao_frame_tiles": st.sao_tiles}
    for name, call in calls.items():
        for edit, g in bad_grids(api, w, h):
            assert call(grid=g.ctypes.data) == INVALID, "%s: %s" % (name, edit)
            assert name.encode() in L.kvz_hip_last_error()
    # and what the untiled entries refuse
    rcs = [st.intra_tiles(cus=None), st.intra_tiles(modes=None), st.intra_tiles(prm=None), st.intra_tiles(table=None), st.intra_tiles(y=None),
           st.intra_tiles(cy=st.ptr("coeff", 0) + 2), st.intra_tiles(cus=st.ptr("cus") + 2), st.intra_tiles(sy=w - 1), st.intra_tiles(u=None),
           st.cu_qp_tiles(0, cus=None), st.cu_qp_tiles(0, cbf=None), st.cu_qp_tiles(0, lcu_qp=None), st.cu_qp_tiles(0, last=None), st.cu_qp_tiles(0, prm=None),
           st.cu_qp_tiles(0, cus=st.ptr("cus") + 2), st.cu_qp_tiles(0, w=w - 4), st.cu_qp_tiles(0, h=4), st.cu_qp_tiles(0, start_qp=-1),
           st.cu_qp_tiles(0, start_qp=52), st.cu_qp_tiles(2), st.cu_qp_tiles(-1),
           st.deblock_tiles(y=None), st.deblock_tiles(cus=None), st.deblock_tiles(prm=None), st.deblock_tiles(w=w - 4), st.deblock_tiles(h=0),
           st.deblock_tiles(sy=w - 4), st.deblock_tiles(sy=w + 2), st.deblock_tiles(y=st.ptr("rec", 0) + 1), st.deblock_tiles(u=None), st.deblock_tiles(sc=w // 2 - 4),
           st.sao_tiles(luma=None), st.sao_tiles(chro=None), st.sao_tiles(y=None), st.sao_tiles(dy=None), st.sao_tiles(dy=st.ptr("rec", 0)),
           st.sao_tiles(du=st.ptr("rec", 1)), st.sao_tiles(w=w + 4), st.sao_tiles(h=4), st.sao_tiles(sy=w - 4), st.sao_tiles(y=st.ptr("rec", 0) + 2),
           st.sao_tiles(luma=st.ptr("sao", 0) + 2)]
    assert rcs == [INVALID] * len(rcs), rcs
    st.sync()
    got = st.result()
    for k in range(3):
        np.testing.assert_array_equal(got["rec"][k], case["pred"][k])
        assert (got["dst"][k] == POISON_DST).all()
        np.testing.assert_array_equal(got["coeff"][k], init[0][k])
    np.testing.assert_array_equal(got["cus"].view(np.uint8), case["cus"].view(np.uint8))
    assert (got["cbf_out"] == 0x5D).all() and (got["last"] == QL.POISON_LAST).all()
    np.testing.assert_array_equal(got["costs"].view(np.uint32), init[2].view(np.uint32))
    assert L.kvz_hip_abi_version() == 4
    # 47 tile columns are a grid: a picture 47 LCUs wide, every LCU column a tile
    wide = api.tile_grid(47 * 64, 64, list(range(48)), [0, 1])
    cus = np.zeros((16, 47 * 16), dtype=TC.CU_INFO)
    got_cus, last = api.cu_qp_frame_tiles(cus, np.zeros(cus.shape, np.uint8), np.arange(47, dtype=np.int8), 33, wide)
    assert (last == 33).all() and (got_cus["qp"] == 33).all()


# ---------------------------------------------------------------- 7. the numpy conveniences
@pytest.mark.parametrize("pic", TC.FIXTURE_PICTURES[::2], ids=[p[0] for p in TC.FIXTURE_PICTURES[::2]])
def test_numpy_conveniences_with_tiles(api, pic):
    case, want = TC.load_fixture_case(np.load(GOLDEN, allow_pickle=False), pic)
    w, h, chroma = case["width"], case["height"], case["chroma"]
    g = api.tile_grid(w, h, case["col_bd"], case["row_bd"])
    init = QC.zero_outputs(w, h, chroma)
    mid = api.inter_residual_frame(case["src"], case["pred"], case["cus"], QC.PARAMS_QP, chroma, case["slice_is_intra"], case["signhide"], coeff=init[0],
                                   cbf_out=init[1], costs=init[2], lcu_qp=case["lcu_qp"])
    full = api.intra_recon_frame(case["src"], mid["rec"], mid["cus"], case["modes"], QC.PARAMS_QP, chroma, case["signhide"], case["slice_is_intra"],
                                 coeff=mid["coeff"], cbf_out=mid["cbf_out"], costs=mid["costs"], lcu_qp=case["lcu_qp"], tiles=g)
    QC.assert_outputs_equal(full, want["full"], case["name"] + " convenience", chroma)
    for rows in (0, 1):
        cus, last = api.cu_qp_frame_tiles(full["cus"], full["cbf_out"], case["lcu_qp"], case["start_qp"], g, chain_rows=rows)
        np.testing.assert_array_equal(cus.view(np.uint8), want["cus_qp_rows" if rows else "cus_qp"].view(np.uint8))
        np.testing.assert_array_equal(last, want["last_rows" if rows else "last"])
    cus, _ = api.cu_qp_frame_tiles(full["cus"], full["cbf_out"], case["lcu_qp"], case["start_qp"], g)
    deb = api.deblock_frame(full["rec"][0], full["rec"][1], full["rec"][2], cus, TC.chain_deblock_params(case), tiles=g)
    assert_planes(deb, want["deb"], "deblock_frame(tiles=)")
    dst = api.sao_frame(deb, case["sao_luma"], case["sao_chroma"], chroma, tiles=g)
    assert_planes(dst, want["sao"], "sao_frame(tiles=)")
    # uniform_tile_grid is tile_grid with the reference's spacing
    u = api.uniform_tile_grid(w, h, 2, 2)
    lx, ly = QC.lcu_grid(w, h)
    assert u.tobytes() == api.tile_grid(w, h, TC.uniform_bd(lx, 2), TC.uniform_bd(ly, 2)).tobytes()

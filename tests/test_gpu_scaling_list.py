"""GPU: the scaling-list entries of the picture chain -- kvz_hip_inter_residual_frame_sl and kvz_hip_intra_recon_frame_sl -- against the
committed fixture (tests/scaling_list_cases.py: the reference's default lists through its own scaling-list path, a custom set through
the oracle's table path); against the entries without lists, with no tables and with all-16 lists; on odd strides and offset planes;
replayed from a captured graph after the tables changed; in the chain up to deblocking; and for what they refuse.  Every output starts
poisoned, every array -- the tables included -- is staged between guard bands, every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import inter_residual_cases as RC
import lcu_qp_cases as QC
import scaling_list_cases as SL
import test_gpu_inter_residual as TR
import test_gpu_lcu_qp as QL

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaling_list.npz")
INVALID = -2
PICS = {p[0]: p for p in SL.FIXTURE_PICTURES}


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


check = QL.check


class Staged(QL.Staged):
    """the staging of the per-LCU-QP tests plus the two packed arrays, the kvz_hip_scaling_tables struct and the grid.  tables None:
    params->scaling_list = 0 and no struct.  pad: extra columns of every plane (odd strides) and, for the planes the entries write,
    a start `pad` bytes into the first row (offset planes)"""

    def __init__(self, A, case, tables, init=None, pad=0):
        from kvazaar_amd import _lib
        w, h, chroma = case["width"], case["height"], case["chroma"]
        self.pad = pad
        src, pred = case["src"], case["pred"]
        if pad:
            src = tuple(None if p is None else self._padded(p, 0) for p in src)
            pred = tuple(None if p is None else self._padded(p, pad) for p in pred)
        QL.Staged.__init__(self, A, src, pred, case["cus"], case["modes"], case["lcu_qp"], case["qp"], chroma, case["signhide"], case["slice_is_intra"],
                           init=init or QC.zero_outputs(w, h, chroma))
        self.w, self.h = w, h
        self.table = A.ref_picture_table([(self.ptr("src", 0), self.ptr("src", 1), self.ptr("src", 2), self.host["src"][0].shape[1],
                                           self.host["src"][1].shape[1] if chroma else 0)], w, h)
        self.prm = A.inter_residual_params(case["qp"], case["slice_is_intra"], case["signhide"], chroma, 0 if tables is None else 1)
        self.per_lcu = case["per_lcu"]
        self.grid = A.tile_grid(w, h, case["col_bd"], case["row_bd"]) if case["tiled"] else None
        self.sl = None
        if tables is not None:
            self.host["tables"] = [np.ascontiguousarray(t, dtype=np.int32) for t in tables]
            self.dev["tables"] = [self._up(a) for a in self.host["tables"]]
            self.sl = _lib.ScalingTables(self.ptr("tables", 0), self.ptr("tables", 1))
        self.dprm = SL.chain_deblock_params(case)

    def _padded(self, p, lead):
        a = np.full((p.shape[0], p.shape[1] + 2 * self.pad + 1), RC.POISON_PIXEL, np.uint8)
        a[:, lead:lead + p.shape[1]] = p
        return a

    def sl_args(self, over):
        a = self.args(over)
        if self.pad:
            for k in ("y", "u", "v"):
                if a[k] is not None and k not in over:
                    a[k] += self.pad
        a.setdefault("lcu_qp", self.qp_ptr() if self.per_lcu else None)
        a.setdefault("grid", self.grid.ctypes.data if self.grid is not None else None)
        a.setdefault("tables", C.byref(self.sl) if self.sl is not None else None)
        return a

    def inter_sl(self, stream=None, **over):
        a = self.sl_args(over)
        return self.L.kvz_hip_inter_residual_frame_sl(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["cy"], a["cu"], a["cv"], a["cbf"],
                                                      a["costs"], a["lcu_qp"], a["tables"], a["prm"], stream)

    def intra_sl(self, stream=None, **over):
        a = self.sl_args(over)
        return self.L.kvz_hip_intra_recon_frame_sl(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["modes"], a["cy"], a["cu"], a["cv"],
                                                   a["cbf"], a["costs"], a["lcu_qp"], a["grid"], a["tables"], a["prm"], stream)

    def inter_plain(self, stream=None):
        a = self.sl_args({})
        return self.L.kvz_hip_inter_residual_frame_qp(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["cy"], a["cu"], a["cv"], a["cbf"],
                                                      a["costs"], a["lcu_qp"], a["prm"], stream)

    def intra_plain(self, stream=None):
        a = self.sl_args({})
        return self.L.kvz_hip_intra_recon_frame_tiles(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["modes"], a["cy"], a["cu"], a["cv"],
                                                      a["cbf"], a["costs"], a["lcu_qp"], a["grid"], a["prm"], stream)

    def deblock(self, stream=None):
        a = self.sl_args({})
        return self.L.kvz_hip_deblock_frame(a["y"], a["sy"], a["u"], a["v"], a["sc"], self.w, self.h, a["cus"], self.dprm.ctypes.data, stream)

    def sync(self, stream=None):
        check(self.L.kvz_hip_stream_sync(stream), "sync")

    def result(self):
        """asserts every guard band, the source, the modes, the QP array and the tables; with pad: the planes cut to the picture, after
        asserting that nothing around it was written"""
        out = QL.Staged.result(self)
        for k, t in enumerate(self.host.get("tables", [])):
            np.testing.assert_array_equal(self.raw("tables", k)[TR.GUARD:-TR.GUARD].view(np.int32), t, err_msg="the tables were written")
        if self.pad:
            cut = []
            for k, p in enumerate(out["rec"]):
                if p is None:
                    cut.append(None)
                    continue
                pw = self.w >> (1 if k else 0)
                outside = np.ones(p.shape, bool)
                outside[:, self.pad:self.pad + pw] = False
                assert (p[outside] == RC.POISON_PIXEL).all(), "wrote outside the picture of plane %d" % k
                cut.append(p[:, self.pad:self.pad + pw])
            out["rec"] = tuple(cut)
        return out


def run_both(st, stream=None):
    check(st.inter_sl(stream), "inter_residual_frame_sl")
    check(st.intra_sl(stream), "intra_recon_frame_sl")


# ---------------------------------------------------------------- 1. the fixture, entry by entry
@pytest.mark.parametrize("which", SL.LIST_SETS)
@pytest.mark.parametrize("name", list(PICS))
def test_fixture_through_both_entries(api, golden, name, which):
    case = SL.load_case(golden, PICS[name])
    chroma = case["chroma"]
    st = Staged(api, case, SL.load_tables(golden, which))
    check(st.inter_sl(), "inter_residual_frame_sl")
    st.sync()
    SL.assert_outputs_equal(st.result(), SL.load_want(golden, name, which, "mid", chroma), "%s %s inter" % (name, which), chroma)
    check(st.intra_sl(), "intra_recon_frame_sl")
    st.sync()
    got = st.result()
    SL.assert_outputs_equal(got, SL.load_want(golden, name, which, "full", chroma), "%s %s intra" % (name, which), chroma)
    assert (got["last"] == QL.POISON_LAST).all()


def test_numpy_conveniences_route_to_the_entries(api, golden):
    for name in ("ragged", "mono"):
        case = SL.load_case(golden, PICS[name])
        chroma, w, h = case["chroma"], case["width"], case["height"]
        init = QC.zero_outputs(w, h, chroma)
        lq = case["lcu_qp"] if case["per_lcu"] else None
        tables = SL.load_tables(golden, "custom")
        mid = api.inter_residual_frame(case["src"], case["pred"], case["cus"], case["qp"], chroma, case["slice_is_intra"], case["signhide"], coeff=init[0],
                                       cbf_out=init[1], costs=init[2], lcu_qp=lq, scaling=tables)
        SL.assert_outputs_equal(mid, SL.load_want(golden, name, "custom", "mid", chroma), name + " inter convenience", chroma)
        tiles = api.tile_grid(w, h, case["col_bd"], case["row_bd"]) if case["tiled"] else None
        full = api.intra_recon_frame(case["src"], mid["rec"], mid["cus"], case["modes"], case["qp"], chroma, case["signhide"], case["slice_is_intra"],
                                     coeff=mid["coeff"], cbf_out=mid["cbf_out"], costs=mid["costs"], lcu_qp=lq, tiles=tiles, scaling=tables)
        SL.assert_outputs_equal(full, SL.load_want(golden, name, "custom", "full", chroma), name + " intra convenience", chroma)


# ---------------------------------------------------------------- 2. without tables: the _qp / _tiles entries
@pytest.mark.parametrize("name", ["ragged", "hide"])
def test_null_tables_are_the_entries_without_lists_byte_for_byte(api, golden, name):
    """ragged: a QP per LCU and tiles; hide: lcu_qp == NULL and grid == NULL"""
    case = SL.load_case(golden, PICS[name])
    old = Staged(api, case, None)
    check(old.inter_plain(), "inter_residual_frame_qp")
    check(old.intra_plain(), "intra_recon_frame_tiles")
    old.sync()
    want = old.result()
    assert any((c != RC.POISON_COEFF).any() and c.any() for c in want["coeff"] if c is not None)
    new = Staged(api, case, None)
    run_both(new)
    new.sync()
    SL.assert_outputs_equal(new.result(), want, name + " tables == NULL", case["chroma"])
    # and the lists matter
    assert not np.array_equal(want["coeff"][0], golden[name + "_default_full_coeff_y"])


# ---------------------------------------------------------------- 3. all-16 lists: the flat entries' outputs
@pytest.mark.parametrize("name", list(PICS))
def test_lists_of_sixteen_equal_the_flat_entries(api, golden, name):
    """flat tables are quant_scales and inv_quant_scales << 4: the table path and the flat path must agree at every QP of the fixture
    (0 mod 6 to 5 mod 6, both dequantisation branches), with and without sign hiding"""
    case = SL.load_case(golden, PICS[name])
    flat = SL.process_lists([np.full((SL.LIST_NUM[s], 16 if s == 0 else 64), 16, np.int32) for s in range(4)], np.zeros((4, 6), np.int32))
    q, d = SL.dense(flat)
    at = SL.table_offset(2, 4, 3)
    assert q[at] == 18396 and d[at] == 57 << 4 and len(set(q[at:at + 256].tolist())) == 1
    old = Staged(api, case, None)
    check(old.inter_plain(), "inter_residual_frame_qp")
    check(old.intra_plain(), "intra_recon_frame_tiles")
    old.sync()
    new = Staged(api, case, (q, d))
    run_both(new)
    new.sync()
    SL.assert_outputs_equal(new.result(), old.result(), name + " all-16 lists", case["chroma"])


# ---------------------------------------------------------------- 4. the PLANES rule
def test_odd_strides_and_offset_planes(api, golden):
    case = SL.load_case(golden, PICS["ragged"])
    st = Staged(api, case, SL.load_tables(golden, "custom"), pad=3)
    assert st.host["rec"][0].shape[1] == 207 and st.host["rec"][1].shape[1] == 107 and st.host["src"][0].shape[1] == 207
    run_both(st)
    st.sync()
    SL.assert_outputs_equal(st.result(), SL.load_want(golden, "ragged", "custom", "full", 1), "odd strides", 1)


# ---------------------------------------------------------------- 5. capture
def test_captured_calls_replay_after_the_tables_changed(api, golden):
    case = SL.load_case(golden, PICS["ragged"])
    st = Staged(api, case, SL.load_tables(golden, "default"))
    L, s, graph = st.L, st.L.kvz_hip_stream_create(), C.c_void_p()
    check(L.kvz_hip_graph_begin(s), "graph_begin")
    run_both(st, s)
    check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
    assert graph.value
    try:
        for which in ("default", "custom", "default"):
            tables = SL.load_tables(golden, which)
            for k in range(2):
                st.upload("tables", k, tables[k], s)
            st.host["tables"] = [np.ascontiguousarray(t, dtype=np.int32) for t in tables]
            for kind in ("rec", "coeff", "cus", "cbf_out", "costs"):
                for k, a in enumerate(st.host[kind]):
                    st.upload(kind, k, a, s)
            st.sync(s)
            check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            st.sync(s)
            SL.assert_outputs_equal(st.result(), SL.load_want(golden, "ragged", which, "full", 1), "replayed with the %s lists" % which, 1)
    finally:
        L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


# ---------------------------------------------------------------- 6. refusals
def test_refusals_name_the_entry_and_write_nothing(api, golden):
    from kvazaar_amd import _lib
    case = SL.load_case(golden, PICS["ragged"])
    w, h, chroma = case["width"], case["height"], case["chroma"]
    st = Staged(api, case, SL.load_tables(golden, "custom"))
    L = st.L
    flat = api.inter_residual_params(case["qp"], 0, 0, chroma, scaling_list=0)
    no_q, no_d = _lib.ScalingTables(None, st.ptr("tables", 1)), _lib.ScalingTables(st.ptr("tables", 0), None)
    off_q, off_d = _lib.ScalingTables(st.ptr("tables", 0) + 4, st.ptr("tables", 1)), _lib.ScalingTables(st.ptr("tables", 0), st.ptr("tables", 1) + 8)
    bad_grid = api.tile_grid(w, h, case["col_bd"], case["row_bd"])
    bad_grid["col_bd"][0, 1] = 0
    negative = api.inter_residual_params(-1, 0, 0, chroma, scaling_list=1)
    for call, entry in ((st.inter_sl, b"kvz_hip_inter_residual_frame_sl"), (st.intra_sl, b"kvz_hip_intra_recon_frame_sl")):
        overs = [{"prm": flat.ctypes.data}, {"tables": None}, {"tables": C.byref(no_q)}, {"tables": C.byref(no_d)}, {"tables": C.byref(off_q)},
                 {"tables": C.byref(off_d)}, {"prm": None}, {"table": None}, {"cus": None}, {"cy": st.ptr("coeff", 0) + 2}, {"sy": w - 1},
                 {"prm": negative.ctypes.data, "lcu_qp": None}]
        if call == st.intra_sl:
            overs += [{"modes": None}, {"grid": bad_grid.ctypes.data}]
        for over in overs:
            assert call(**over) == INVALID, (entry, sorted(over))
            assert entry in L.kvz_hip_last_error(), (entry, sorted(over), L.kvz_hip_last_error())
    st.sync()
    init = QC.zero_outputs(w, h, chroma)
    untouched = {"rec": case["pred"], "coeff": init[0], "cus": case["cus"], "cbf_out": init[1], "costs": init[2]}
    SL.assert_outputs_equal(st.result(), untouched, "after refused calls", chroma)
    # the entries without lists keep refusing scaling_list != 0
    assert st.inter_plain() == INVALID and b"kvz_hip_inter_residual_frame_qp" in L.kvz_hip_last_error()
    assert st.intra_plain() == INVALID and b"kvz_hip_intra_recon_frame_tiles" in L.kvz_hip_last_error()
    st.sync()
    SL.assert_outputs_equal(st.result(), untouched, "after refused calls", chroma)
    assert L.kvz_hip_abi_version() == 4


# ---------------------------------------------------------------- 7. the chain up to deblocking
def test_chain_to_deblocking_on_one_stream(api, golden):
    """_sl inter -> _sl intra -> kvz_hip_cu_qp_frame -> kvz_hip_deblock_frame (per_cu_qp = 1) on `ragged` without tiles"""
    case = SL.load_case(golden, PICS["ragged"])
    case["tiled"] = False
    st = Staged(api, case, SL.load_tables(golden, "custom"))
    s = st.L.kvz_hip_stream_create()
    try:
        run_both(st, s)
        check(st.cu_qp(SL.CHAIN_START_QP, 0, s), "cu_qp_frame")
        check(st.deblock(s), "deblock_frame")
        st.sync(s)
        got = st.result()
    finally:
        st.L.kvz_hip_stream_destroy(s)
    for k, n in enumerate("yuv"):
        np.testing.assert_array_equal(got["rec"][k], golden["ragged_chain_deb_" + n], err_msg="deblocked plane " + n)
    np.testing.assert_array_equal(got["cus"].view(np.uint8).reshape(golden["ragged_chain_cus"].shape), golden["ragged_chain_cus"])
    np.testing.assert_array_equal(got["last"], golden["ragged_chain_last"])
    # tiles matter to this picture: the untiled intra stage differs from the fixture's tiled one
    assert not np.array_equal(got["coeff"][0], golden["ragged_custom_full_coeff_y"])

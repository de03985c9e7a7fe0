"""GPU: the transform-skip entries of the picture chain -- kvz_hip_inter_residual_frame_ts and kvz_hip_intra_recon_frame_ts -- against
the committed fixture (tests/trskip_cases.py: both trials from the reference's own kvz_quantize_residual, the decision restated);
against the _sl entries with ts == NULL; at bit costs where |coeff| or the SSD alone decides; with a bit cost per LCU; on odd strides,
offset planes and a tr_skip_out at an odd address; replayed from a captured graph after the bit costs and the source changed; in the
chain up to deblocking; and for what they refuse.  Every output starts poisoned, every array is staged between guard bands, every
comparison is exact.  Every test runs under a time limit of its own that ends the process (a hung call cannot be interrupted from
Python), and after a call or a synchronisation that reports a runtime error no further test starts anything on the device."""
import ctypes as C
import faulthandler
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from lcu_qp_cases import zero_outputs
import scaling_list_cases as SL
import test_gpu_inter_residual as TR
import test_gpu_scaling_list as GS
import trskip_cases as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "trskip.npz")
INVALID = -2
PICS = {p[0]: p for p in T.FIXTURE_PICTURES}
TEST_LIMIT_S = 60                                                     # every test takes a fraction of a second
FAULTS = []


def check(rc, what):
    try:
        GS.check(rc, what)
    except Exception:
        FAULTS.append(what)
        raise


@pytest.fixture(autouse=True)
def limits():
    assert not FAULTS, "an earlier test met a device error (%s): nothing more is started" % FAULTS[0]
    faulthandler.dump_traceback_later(TEST_LIMIT_S, exit=True, file=sys.__stderr__)   # the real stderr under every capture mode
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def lists():
    """the reference's processed default lists: (packed pair for the device, tables for the oracle)"""
    z = np.load(GS.GOLDEN, allow_pickle=False)
    return (z["default_quant"], z["default_dequant"]), SL.undense(z["default_quant"], z["default_dequant"])


def tables_for(case, lists):
    return lists[0] if case["lists"] else None


class Staged(GS.Staged):
    """the staging of the scaling-list tests plus the bit costs, the kvz_hip_trskip struct and tr_skip_out, which starts poisoned and
    one byte into its buffer where odd: an odd address.  bit_cost: an int, or an array for lcu_bit_cost (default: the case's)"""

    def __init__(self, A, case, tables, bit_cost=None, odd=True, pad=0):
        from kvazaar_amd import _lib
        GS.Staged.__init__(self, A, case, tables, pad=pad)
        self.odd = 1 if odd else 0
        bit_cost = case["bit_cost"] if bit_cost is None else bit_cost
        self.host["tr_skip"] = [np.full(case["cus"].size + self.odd, T.POISON_SKIP, np.uint8)]
        lcus = np.asarray(case["lcu_qp"]).size
        self.host["bit_cost"] = [np.asarray(bit_cost, np.int32).reshape(lcus) if np.ndim(bit_cost) else np.full(lcus, -77, np.int32)]
        for k in ("tr_skip", "bit_cost"):
            self.dev[k] = [self._up(self.host[k][0])]
        self.ts = _lib.TrSkip(0 if np.ndim(bit_cost) else int(bit_cost), 0, self.ptr("bit_cost") if np.ndim(bit_cost) else None)
        self.tprm = np.zeros(1, dtype=A.CU_QP_TILES_PARAMS)

    def ts_args(self, over):
        a = self.sl_args(over)
        a.setdefault("ts", C.byref(self.ts))
        a.setdefault("skip", self.ptr("tr_skip") + self.odd)
        return a

    def inter_ts(self, stream=None, **over):
        a = self.ts_args(over)
        return self.L.kvz_hip_inter_residual_frame_ts(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["cy"], a["cu"], a["cv"], a["cbf"],
                                                      a["costs"], a["lcu_qp"], a["tables"], a["ts"], a["skip"], a["prm"], stream)

    def intra_ts(self, stream=None, **over):
        a = self.ts_args(over)
        return self.L.kvz_hip_intra_recon_frame_ts(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["modes"], a["cy"], a["cu"], a["cv"],
                                                   a["cbf"], a["costs"], a["lcu_qp"], a["grid"], a["tables"], a["ts"], a["skip"], a["prm"], stream)

    def cu_qp_tiles(self, start_qp, stream=None):
        self.tprm["start_qp"], self.tprm["chain_rows"] = start_qp, 0
        return self.L.kvz_hip_cu_qp_frame_tiles(self.ptr("cus"), self.ptr("cbf_out"), self.w, self.h, self.qp_ptr(), self.ptr("last"),
                                                self.grid.ctypes.data, self.tprm.ctypes.data, stream)

    def deblock_tiles(self, stream=None):
        a = self.sl_args({})
        return self.L.kvz_hip_deblock_frame_tiles(a["y"], a["sy"], a["u"], a["v"], a["sc"], self.w, self.h, a["cus"], self.grid.ctypes.data,
                                                  self.dprm.ctypes.data, stream)

    def sync(self, stream=None):
        check(self.L.kvz_hip_stream_sync(stream), "sync")

    def result(self):
        """asserts every guard band, every input and the byte before an odd tr_skip_out"""
        out = GS.Staged.result(self)
        np.testing.assert_array_equal(self.raw("bit_cost", 0)[TR.GUARD:-TR.GUARD].view(np.int32), self.host["bit_cost"][0], err_msg="the bit costs were written")
        s = self.raw("tr_skip", 0)[TR.GUARD:-TR.GUARD]
        assert (s[:self.odd] == T.POISON_SKIP).all()
        out["tr_skip"] = s[self.odd:].reshape(self.host["cus"][0].shape)
        return out


def run_both(st, stream=None):
    check(st.inter_ts(stream), "inter_residual_frame_ts")
    check(st.intra_ts(stream), "intra_recon_frame_ts")


def composed(case, lists, **kw):
    return T.compose(case, O, lists[1], **kw)


# ---------------------------------------------------------------- 1. the fixture, entry by entry
@pytest.mark.parametrize("odd", [True, False])
@pytest.mark.parametrize("name", list(PICS))
def test_fixture_through_both_entries(api, golden, lists, name, odd):
    """tr_skip_out keeps its poison outside the entry's CUs and outside 4x4 luma TUs: the fixture's map holds it there"""
    case = T.load_case(golden, PICS[name])
    chroma = case["chroma"]
    st = Staged(api, case, tables_for(case, lists), odd=odd)
    check(st.inter_ts(), "inter_residual_frame_ts")
    st.sync()
    want = T.load_want(golden, name, "mid", chroma)
    T.assert_outputs_equal(st.result(), want, "%s inter" % name, chroma)
    check(st.intra_ts(), "intra_recon_frame_ts")
    st.sync()
    want = T.load_want(golden, name, "full", chroma)
    T.assert_outputs_equal(st.result(), want, "%s intra" % name, chroma)
    assert (want["tr_skip"] == T.POISON_SKIP).any() and (want["tr_skip"] == 1).any() and (want["tr_skip"] == 0).any()


def test_numpy_conveniences_route_to_the_entries(api, golden, lists):
    for name in ("mixed", "mono"):
        case = T.load_case(golden, PICS[name])
        chroma, w, h = case["chroma"], case["width"], case["height"]
        lq = case["lcu_qp"] if case["per_lcu"] else None
        poison = np.full(case["cus"].shape, T.POISON_SKIP, np.uint8)
        init = zero_outputs(w, h, chroma)
        mid = api.inter_residual_frame(case["src"], case["pred"], case["cus"], case["qp"], chroma, case["slice_is_intra"], case["signhide"], coeff=init[0],
                                       cbf_out=init[1], costs=init[2], lcu_qp=lq, scaling=tables_for(case, lists), trskip=case["bit_cost"], tr_skip=poison)
        T.assert_outputs_equal(mid, T.load_want(golden, name, "mid", chroma), name + " inter convenience", chroma)
        tiles = api.tile_grid(w, h, case["col_bd"], case["row_bd"]) if case["tiled"] else None
        full = api.intra_recon_frame(case["src"], mid["rec"], mid["cus"], case["modes"], case["qp"], chroma, case["signhide"], case["slice_is_intra"],
                                     coeff=mid["coeff"], cbf_out=mid["cbf_out"], costs=mid["costs"], lcu_qp=lq, tiles=tiles,
                                     scaling=tables_for(case, lists), trskip=case["bit_cost"], tr_skip=mid["tr_skip"])
        T.assert_outputs_equal(full, T.load_want(golden, name, "full", chroma), name + " intra convenience", chroma)


# ---------------------------------------------------------------- 2. without ts: the _sl entries
@pytest.mark.parametrize("name", ["mixed", "mono"])
def test_null_ts_is_the_sl_entry_byte_for_byte(api, golden, lists, name):
    """mixed: tables, a QP per LCU and tiles; mono: none of them"""
    case = T.load_case(golden, PICS[name])
    old = Staged(api, case, tables_for(case, lists))
    GS.run_both(old)
    old.sync()
    want = old.result()
    assert (want["tr_skip"] == T.POISON_SKIP).all()
    new = Staged(api, case, tables_for(case, lists))
    check(new.inter_ts(ts=None), "inter_residual_frame_ts")
    check(new.intra_ts(ts=None, skip=None), "intra_recon_frame_ts")
    new.sync()
    T.assert_outputs_equal(new.result(), want, name + " ts == NULL", case["chroma"])
    # and transform skip matters
    assert not np.array_equal(want["coeff"][0], golden[name + "_full_coeff_y"])


# ---------------------------------------------------------------- 3. the two ends of the bit cost
@pytest.mark.parametrize("bit_cost", [0, 1 << 21])
def test_bit_cost_zero_and_very_large(api, golden, lists, bit_cost):
    """0: the SSD alone decides.  2^21 is above any difference of two SSDs of a 4x4 block (16 * 255^2 < 2^21): the transformed trial
    is kept wherever the skipped one has the larger coefficient cost"""
    for name in ("inter", "intra"):
        case = T.load_case(golden, PICS[name])
        st = Staged(api, case, None, bit_cost=bit_cost)
        run_both(st)
        st.sync()
        mid, full = composed(case, lists, bit_cost=bit_cost)
        T.assert_outputs_equal(st.result(), full, "%s at bit cost %d" % (name, bit_cost), case["chroma"])
        log = mid["log"] + full["log"]
        assert {0, 1} <= {r["skip"] for r in log}
        assert not np.array_equal(full["tr_skip"], golden[name + "_full_tr_skip"])


# ---------------------------------------------------------------- 4. a bit cost per LCU
def test_lcu_bit_cost_against_a_scalar(api, golden, lists):
    case = T.load_case(golden, PICS["mixed"])
    scalar = T.lambda_bit_cost(case["qp"])
    runs = []
    for bc in (scalar, np.full(6, scalar, np.int32), case["bit_cost"]):
        st = Staged(api, case, lists[0], bit_cost=bc)
        run_both(st)
        st.sync()
        runs.append(st.result())
    T.assert_outputs_equal(runs[1], runs[0], "a constant lcu_bit_cost", 1)
    assert (runs[2]["tr_skip"] != runs[0]["tr_skip"]).any()
    T.assert_outputs_equal(runs[2], T.load_want(golden, "mixed", "full", 1), "lcu_bit_cost", 1)
    # negative values count as 0
    mono = T.load_case(golden, PICS["mono"])
    a, b = Staged(api, mono, None, bit_cost=np.array([-5, -1, -(1 << 31), -9], np.int32)), Staged(api, mono, None, bit_cost=0)
    for st in (a, b):
        run_both(st)
        st.sync()
    T.assert_outputs_equal(a.result(), b.result(), "negative lcu_bit_cost", 0)


# ---------------------------------------------------------------- 5. the PLANES rule
def test_odd_strides_and_offset_planes(api, golden, lists):
    case = T.load_case(golden, PICS["mixed"])
    st = Staged(api, case, lists[0], pad=3)
    assert st.host["rec"][0].shape[1] == 143 and st.host["rec"][1].shape[1] == 75 and st.host["src"][0].shape[1] == 143
    run_both(st)
    st.sync()
    T.assert_outputs_equal(st.result(), T.load_want(golden, "mixed", "full", 1), "odd strides", 1)


# ---------------------------------------------------------------- 6. capture
def test_captured_calls_replay_after_the_bit_costs_and_the_source_changed(api, golden, lists):
    case = T.load_case(golden, PICS["mixed"])
    other = dict(case, src=tuple(np.ascontiguousarray(p[::-1, ::-1]) for p in case["src"]), bit_cost=np.array(case["bit_cost"][::-1]))
    wants = {"first": T.load_want(golden, "mixed", "full", 1), "other": composed(other, lists)[1]}
    assert not np.array_equal(wants["first"]["tr_skip"], wants["other"]["tr_skip"])
    st = Staged(api, case, lists[0])
    L, s, graph = st.L, st.L.kvz_hip_stream_create(), C.c_void_p()
    check(L.kvz_hip_graph_begin(s), "graph_begin")
    run_both(st, s)
    check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
    assert graph.value
    try:
        for which, c in (("first", case), ("other", other), ("first", case)):
            for k, p in enumerate(c["src"]):
                st.upload("src", k, p, s)
            st.host["src"] = [np.ascontiguousarray(p) for p in c["src"]]
            st.upload("bit_cost", 0, np.asarray(c["bit_cost"], np.int32), s)
            st.host["bit_cost"] = [np.asarray(c["bit_cost"], np.int32)]
            for kind in ("rec", "coeff", "cus", "cbf_out", "costs", "tr_skip"):
                for k, a in enumerate(st.host[kind]):
                    st.upload(kind, k, a, s)
            st.sync(s)
            check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            st.sync(s)
            T.assert_outputs_equal(st.result(), wants[which], "replayed on the %s picture" % which, 1)
    finally:
        L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


# ---------------------------------------------------------------- 7. refusals
def test_refusals_name_the_entry_and_write_nothing(api, golden, lists):
    from kvazaar_amd import _lib
    case = T.load_case(golden, PICS["mixed"])
    w, h, chroma = case["width"], case["height"], case["chroma"]
    st = Staged(api, case, lists[0])
    L = st.L
    flat = api.inter_residual_params(case["qp"], 0, 0, chroma, scaling_list=0)
    negative = _lib.TrSkip(-1, 0, None)
    odd_array = _lib.TrSkip(0, 0, st.ptr("bit_cost") + 2)
    no_q = _lib.ScalingTables(None, st.ptr("tables", 1))
    bad_grid = api.tile_grid(w, h, case["col_bd"], case["row_bd"])
    bad_grid["col_bd"][0, 1] = 0
    for call, entry in ((st.inter_ts, b"kvz_hip_inter_residual_frame_ts"), (st.intra_ts, b"kvz_hip_intra_recon_frame_ts")):
        overs = [{"skip": None}, {"ts": C.byref(negative)}, {"ts": C.byref(odd_array)}, {"prm": flat.ctypes.data}, {"tables": None},
                 {"tables": C.byref(no_q)}, {"prm": None}, {"table": None}, {"cus": None}, {"cy": st.ptr("coeff", 0) + 2}, {"sy": w - 1}]
        if call == st.intra_ts:
            overs += [{"modes": None}, {"grid": bad_grid.ctypes.data}]
        for over in overs:
            assert call(**over) == INVALID, (entry, sorted(over))
            assert entry in L.kvz_hip_last_error(), (entry, sorted(over), L.kvz_hip_last_error())
    # a negative bit_cost next to an array is not read
    ignored = _lib.TrSkip(-1, 0, st.ptr("bit_cost"))
    st.sync()
    init = zero_outputs(w, h, chroma)
    untouched = {"rec": case["pred"], "coeff": init[0], "cus": case["cus"], "cbf_out": init[1], "costs": init[2],
                 "tr_skip": np.full(case["cus"].shape, T.POISON_SKIP, np.uint8)}
    T.assert_outputs_equal(st.result(), untouched, "after refused calls", chroma)
    check(st.inter_ts(ts=C.byref(ignored)), "inter_residual_frame_ts")
    st.sync()
    T.assert_outputs_equal(st.result(), T.load_want(golden, "mixed", "mid", 1), "bit_cost is not read next to an array", 1)
    assert L.kvz_hip_abi_version() == 4


# ---------------------------------------------------------------- 8. the chain up to deblocking
def test_chain_to_deblocking_on_one_stream(api, golden, lists):
    """_ts inter -> _ts intra -> kvz_hip_cu_qp_frame_tiles -> kvz_hip_deblock_frame_tiles (per_cu_qp = 1) on `mixed`"""
    case = T.load_case(golden, PICS["mixed"])
    st = Staged(api, case, lists[0])
    s = st.L.kvz_hip_stream_create()
    try:
        run_both(st, s)
        check(st.cu_qp_tiles(T.CHAIN_START_QP, s), "cu_qp_frame_tiles")
        check(st.deblock_tiles(s), "deblock_frame_tiles")
        st.sync(s)
        got = st.result()
    finally:
        st.L.kvz_hip_stream_destroy(s)
    for k, n in enumerate("yuv"):
        np.testing.assert_array_equal(got["rec"][k], golden["mixed_chain_deb_" + n], err_msg="deblocked plane " + n)
    np.testing.assert_array_equal(got["cus"].view(np.uint8).reshape(golden["mixed_chain_cus"].shape), golden["mixed_chain_cus"])
    np.testing.assert_array_equal(got["last"], golden["mixed_chain_last"])
    np.testing.assert_array_equal(got["tr_skip"], golden["mixed_full_tr_skip"])
    assert not np.array_equal(got["rec"][0], golden["mixed_full_rec_y"]), "deblocking changed the picture"

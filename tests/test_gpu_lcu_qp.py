"""GPU: the per-LCU-QP entries -- kvz_hip_inter_residual_frame_qp, kvz_hip_intra_recon_frame_qp and kvz_hip_cu_qp_frame -- against the
committed fixture and the composition of the reference's own functions (tests/lcu_qp_cases.py), against the one-QP entries where both
must agree, and in the chain residual -> intra -> QP map -> kvz_hip_deblock_frame (per_cu_qp = 1) on one stream, eager and replayed from a
captured graph.  200 x 136 is 4 x 3 LCUs, ragged on both sides: one N = 4 workgroup of the inter kernel spans the four LCUs of a row, each
with its own QP, and the wavefront of the intra kernel has every neighbour relation; 96 x 72 is the 4:0:0 path.  Every output starts
poisoned, every array is staged between guard bands, the QP array stands at an odd address, every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import inter_residual_cases as RC
import lcu_qp_cases as QC
import oracle_lib as O
import test_gpu_inter_residual as TR
import test_gpu_intra_recon as TX
from patterns import deblock_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lcu_qp.npz")
POISON_LAST = 0x77


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


class Staged(TX.Staged):
    """the staging of the one-QP tests plus the QP array (one byte into its buffer: an odd address) and lcu_last_qp"""

    def __init__(self, A, src, rec, cus, modes, lcu_qp, qp=QC.PARAMS_QP, chroma=1, signhide=0, slice_is_intra=0, init=None):
        TX.Staged.__init__(self, A, src, rec, cus, modes, qp, chroma, signhide, slice_is_intra, init)
        lx, ly = QC.lcu_grid(self.w, self.h)
        n = lx * ly
        q = np.full(n + 1, 0x55, np.int8)
        q[1:] = np.asarray(lcu_qp, dtype=np.int8)
        self.host["lcu_qp"] = [q]
        self.host["last"] = [np.full(n, POISON_LAST, np.int8)]
        for k in ("lcu_qp", "last"):
            self.dev[k] = [self._up(self.host[k][0])]
        self.cprm = np.zeros(1, dtype=A.CU_QP_PARAMS)

    def qp_ptr(self):
        return self.ptr("lcu_qp") + 1

    def set_lcu_qp(self, lcu_qp, stream=None):
        q = np.array(self.host["lcu_qp"][0])
        q[1:] = np.asarray(lcu_qp, dtype=np.int8)
        self.upload("lcu_qp", 0, q, stream)
        self.host["lcu_qp"] = [q]

    def inter_qp(self, stream=None, **over):
        a = self.args(over)
        return self.L.kvz_hip_inter_residual_frame_qp(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["cy"], a["cu"], a["cv"], a["cbf"],
                                                      a["costs"], a.get("lcu_qp", self.qp_ptr()), a["prm"], stream)

    def intra_qp(self, stream=None, **over):
        a = self.args(over)
        return self.L.kvz_hip_intra_recon_frame_qp(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["modes"], a["cy"], a["cu"], a["cv"],
                                                   a["cbf"], a["costs"], a.get("lcu_qp", self.qp_ptr()), a["prm"], stream)

    def cu_qp(self, start_qp, chain_lcus=0, stream=None, **over):
        self.cprm["start_qp"], self.cprm["chain_lcus"] = start_qp, chain_lcus
        a = {"cus": self.ptr("cus"), "cbf": self.ptr("cbf_out"), "w": self.w, "h": self.h, "lcu_qp": self.qp_ptr(), "last": self.ptr("last"),
             "prm": self.cprm.ctypes.data}
        a.update(over)
        return self.L.kvz_hip_cu_qp_frame(a["cus"], a["cbf"], a["w"], a["h"], a["lcu_qp"], a["last"], a["prm"], stream)

    def result(self):
        out = TX.Staged.result(self)                                   # asserts every guard band, the source and the modes
        np.testing.assert_array_equal(self.raw("lcu_qp", 0)[TR.GUARD:-TR.GUARD].view(np.int8), self.host["lcu_qp"][0], err_msg="the QP array was written")
        out["last"] = self.raw("last", 0)[TR.GUARD:-TR.GUARD].view(np.int8)
        return out


def check(rc, what):
    from kvazaar_amd import _lib
    _lib.check(rc, what)


def run_residual(A, src, pred, cus, modes, lcu_qp, chroma, signhide, slice_is_intra, init, qp=QC.PARAMS_QP, null=False):
    st = Staged(A, src, pred, cus, modes, lcu_qp, qp, chroma, signhide, slice_is_intra, init=init)
    over = {"lcu_qp": None} if null else {}
    check(st.inter_qp(**over), "inter_residual_frame_qp")
    check(st.intra_qp(**over), "intra_recon_frame_qp")
    check(st.L.kvz_hip_stream_sync(None), "sync")
    return st


@pytest.mark.parametrize("pic", QC.FIXTURE_PICTURES, ids=[p[0] for p in QC.FIXTURE_PICTURES])
def test_fixture_through_both_residual_entries_and_the_qp_map(api, pic):
    name, w, h, chroma, signhide, slice_is_intra, seed, share, start_qp, _ = pic
    z = np.load(GOLDEN, allow_pickle=False)
    src, pred, cus, modes, lcu_qp, want = QC.load_fixture_case(z, name, chroma)
    st = run_residual(api, src, pred, cus, modes, lcu_qp, chroma, signhide, slice_is_intra, QC.zero_outputs(w, h, chroma))
    got = st.result()
    QC.assert_outputs_equal(got, want["full"], name, chroma)
    assert (got["last"] == POISON_LAST).all(), "the residual entries wrote lcu_last_qp"
    for chain, cus_key, last_key in ((0, "cus_qp", "last"), (QC.lcu_grid(w, h)[0], "cus_qp_rows", "last_rows")):
        st.upload("cus", 0, want["full"]["cus"])
        check(st.cu_qp(start_qp, chain), "cu_qp_frame")
        check(st.L.kvz_hip_stream_sync(None), "sync")
        got = st.result()
        np.testing.assert_array_equal(got["cus"].view(np.uint8), want[cus_key].view(np.uint8), err_msg="%s chain_lcus %d" % (name, chain))
        np.testing.assert_array_equal(got["last"], want[last_key], err_msg="%s chain_lcus %d" % (name, chain))
        np.testing.assert_array_equal(got["cbf_out"], want["full"]["cbf_out"])
    # the numpy conveniences, over zeroed outputs
    mid = api.inter_residual_frame(src, pred, cus, QC.PARAMS_QP, chroma, slice_is_intra, signhide, lcu_qp=lcu_qp)
    full = api.intra_recon_frame(src, mid["rec"], mid["cus"], modes, QC.PARAMS_QP, chroma, signhide, slice_is_intra, coeff=mid["coeff"],
                                 cbf_out=mid["cbf_out"], costs=mid["costs"], lcu_qp=lcu_qp)
    _, zero, mapped, last = QC.compose_chain(src, pred, cus, modes, lcu_qp, start_qp, 0, chroma, signhide, slice_is_intra, B=O)
    QC.assert_outputs_equal(full, zero, name + " convenience", chroma)
    got_cus, got_last = api.cu_qp_frame(full["cus"], full["cbf_out"], lcu_qp, start_qp)
    np.testing.assert_array_equal(got_cus.view(np.uint8), mapped.view(np.uint8))
    np.testing.assert_array_equal(got_last, last)


@pytest.mark.parametrize("pic", QC.FIXTURE_PICTURES[:2], ids=[p[0] for p in QC.FIXTURE_PICTURES[:2]])
def test_null_and_uniform_array_are_the_old_entries_byte_for_byte(api, pic):
    name, w, h, chroma, signhide, slice_is_intra = pic[:6]
    src, pred, cus, modes = QC.fixture_case(*pic)
    n = len(pic[9])
    for qp in (22, 37):
        init = RC.initial_outputs(w, h, chroma)
        old = TX.Staged(api, src, pred, cus, modes, qp, chroma, signhide, slice_is_intra, init=init)
        check(old.inter_call(), "inter_residual_frame")
        check(old.call(), "intra_recon_frame")
        check(old.L.kvz_hip_stream_sync(None), "sync")
        want = old.result()
        assert (want["cbf_out"] != RC.POISON_CBF).any() and any((c != RC.POISON_COEFF).any() and c.any() for c in want["coeff"] if c is not None)
        null = run_residual(api, src, pred, cus, modes, [0] * n, chroma, signhide, slice_is_intra, init, qp=qp, null=True).result()
        QC.assert_outputs_equal(null, want, "%s NULL qp %d" % (name, qp), chroma)
        same = run_residual(api, src, pred, cus, modes, [qp] * n, chroma, signhide, slice_is_intra, init, qp=QC.PARAMS_QP).result()
        QC.assert_outputs_equal(same, want, "%s uniform qp %d" % (name, qp), chroma)
        np.testing.assert_array_equal(same["cus"]["qp"], cus["qp"], err_msg="the residual entries wrote cus[].qp")


def test_values_outside_0_51_behave_as_0_and_51(api):
    pic = QC.FIXTURE_PICTURES[0]
    name, w, h, chroma, signhide, slice_is_intra, seed, share, start_qp, _ = pic
    src, pred, cus, modes = QC.fixture_case(*pic)
    wild = np.array([-3, 60, -128, 127, 60, -3, 52, -1, -3, 60, 60, -3], np.int8)
    init = QC.zero_outputs(w, h, chroma)
    a = run_residual(api, src, pred, cus, modes, wild, chroma, signhide, slice_is_intra, init)
    b = run_residual(api, src, pred, cus, modes, QC.clip_qp(wild), chroma, signhide, slice_is_intra, init)
    assert set(QC.clip_qp(wild).tolist()) == {0, 51}
    QC.assert_outputs_equal(a.result(), b.result(), "clamped", chroma)
    for st in (a, b):
        check(st.cu_qp(start_qp, 0), "cu_qp_frame")
    check(a.L.kvz_hip_stream_sync(None), "sync")
    ra, rb = a.result(), b.result()
    np.testing.assert_array_equal(ra["cus"].view(np.uint8), rb["cus"].view(np.uint8))
    np.testing.assert_array_equal(ra["last"], rb["last"])
    assert set(np.unique(ra["cus"]["qp"]).tolist()) <= {0, 51, start_qp} and set(ra["last"].tolist()) <= {0, 51, start_qp}


@pytest.mark.parametrize("geom", [((2, 8, 220), (1, 4, 124), (1, 4, 124)), ((2, 3, 221), (1, 1, 125), (3, 7, 125))], ids=["aligned", "odd"])
def test_padded_strides_and_offset_bases_with_an_odd_qp_address(api, geom):
    """PLANES in kvz_hip.h, as the one-QP entries are held to it: planes inside larger buffers, per plane (rows above, columns left, stride)"""
    z = np.load(GOLDEN, allow_pickle=False)
    name, w, h, chroma, signhide, slice_is_intra = QC.FIXTURE_PICTURES[0][:6]
    assert (name, w, h) == ("ragged", 200, 136)
    src, pred, cus, modes, lcu_qp, want = QC.load_fixture_case(z, name, chroma)
    big_rec, big_src = [], []
    for k, (top, left, stride) in enumerate(geom):
        ph, pw = pred[k].shape
        for planes, out in ((pred, big_rec), (src, big_src)):
            b = np.full((ph + max(g[0] for g in geom) + 2, stride), RC.POISON_PIXEL, np.uint8)
            b[top:top + ph, left:left + pw] = planes[k]
            out.append(b)
    st = Staged(api, big_src, big_rec, cus, modes, lcu_qp, QC.PARAMS_QP, chroma, signhide, slice_is_intra, init=QC.zero_outputs(w, h, chroma))
    assert st.qp_ptr() % 2 == 1
    off = [top * stride + left for (top, left, stride) in geom]
    table = api.ref_picture_table([(st.ptr("src", 0) + off[0], st.ptr("src", 1) + off[1], st.ptr("src", 2) + off[2], geom[0][2], geom[1][2])], w, h)
    over = dict(table=table.ctypes.data, y=st.ptr("rec", 0) + off[0], u=st.ptr("rec", 1) + off[1], v=st.ptr("rec", 2) + off[2], sy=geom[0][2], sc=geom[1][2])
    check(st.inter_qp(**over), "inter_residual_frame_qp")
    check(st.intra_qp(**over), "intra_recon_frame_qp")
    check(st.L.kvz_hip_stream_sync(None), "sync")
    got = st.result()
    planes = []
    for k, (top, left, stride) in enumerate(geom):
        ph, pw = pred[k].shape
        buf = got["rec"][k]
        planes.append(buf[top:top + ph, left:left + pw])
        outside = np.ones(buf.shape, bool)
        outside[top:top + ph, left:left + pw] = False
        assert (buf[outside] == RC.POISON_PIXEL).all(), "plane %d: wrote outside the picture" % k
    got["rec"] = tuple(planes)
    QC.assert_outputs_equal(got, want["full"], "offset planes")


def _known_staged(A, cus, cbf):
    w, h = QC.KNOWN_W, QC.KNOWN_H
    src = RC.smooth_planes(w, h, 1, 1)
    init = (RC.initial_outputs(w, h, 1)[0], cbf, RC.initial_outputs(w, h, 1)[2])
    return Staged(A, src, src, cus, np.zeros(cus.shape + (2,), np.uint8), QC.KNOWN_LCU_QP, init=init)


def test_qp_map_known_answers_in_every_chain_mode(api):
    cus, cbf, one_chain, row_chains = QC.known_map()
    lx = QC.lcu_grid(QC.KNOWN_W, QC.KNOWN_H)[0]
    st = _known_staged(api, cus, cbf)
    two_rows = list(QC.KNOWN_LAST_ONE_CHAIN[:8]) + list(QC.KNOWN_LAST_ROW_CHAINS[8:])
    for chain, want, last in ((0, one_chain, QC.KNOWN_LAST_ONE_CHAIN), (lx, row_chains, QC.KNOWN_LAST_ROW_CHAINS), (2 * lx, None, two_rows),
                              (5 * lx, one_chain, QC.KNOWN_LAST_ONE_CHAIN)):
        st.upload("cus", 0, cus)
        st.upload("last", 0, st.host["last"][0])
        check(st.cu_qp(QC.KNOWN_START, chain), "cu_qp_frame")
        check(st.L.kvz_hip_stream_sync(None), "sync")
        got = st.result()
        assert got["last"].tolist() == list(last), "chain_lcus %d" % chain
        ref_cus, ref_last = QC.set_cu_qps(cus, cbf, QC.KNOWN_LCU_QP, QC.KNOWN_START, chain)
        assert ref_last.tolist() == list(last)
        np.testing.assert_array_equal(got["cus"]["qp"], ref_cus["qp"] if want is None else want, err_msg="chain_lcus %d" % chain)
        back = np.array(got["cus"])
        back["qp"] = cus["qp"]
        np.testing.assert_array_equal(back.view(np.uint8), cus.view(np.uint8), err_msg="something other than qp was written")
    # a depth above 3 counts as 3, type is not read
    other = np.array(cus)
    other["depth"][other["depth"] == 3] = 200
    other["type"] = 0
    st.upload("cus", 0, other)
    check(st.cu_qp(QC.KNOWN_START, 0), "cu_qp_frame")
    check(st.L.kvz_hip_stream_sync(None), "sync")
    np.testing.assert_array_equal(st.result()["cus"]["qp"], one_chain)


def test_qp_map_refused_arguments_write_nothing(api):
    cus, cbf, _, _ = QC.known_map()
    st = _known_staged(api, cus, cbf)
    L, ok = st.L, QC.KNOWN_START
    rcs = [st.cu_qp(ok, cus=None), st.cu_qp(ok, cbf=None), st.cu_qp(ok, lcu_qp=None), st.cu_qp(ok, last=None), st.cu_qp(ok, prm=None),
           st.cu_qp(ok, cus=st.ptr("cus") + 2), st.cu_qp(ok, w=QC.KNOWN_W - 4), st.cu_qp(ok, h=QC.KNOWN_H + 4), st.cu_qp(ok, w=0), st.cu_qp(ok, h=4),
           st.cu_qp(-1), st.cu_qp(52), st.cu_qp(ok, -4), st.cu_qp(ok, 3), st.cu_qp(ok, 6)]
    for rc in rcs:
        assert rc == -2 and b"kvz_hip_cu_qp_frame" in L.kvz_hip_last_error()
    L.kvz_hip_stream_sync(None)
    got = st.result()
    np.testing.assert_array_equal(got["cus"].view(np.uint8), cus.view(np.uint8))
    assert (got["last"] == POISON_LAST).all()
    assert L.kvz_hip_abi_version() == 4
    assert st.cu_qp(0) == 0 and st.cu_qp(51, 4) == 0 and st.cu_qp(ok, 8) == 0
    L.kvz_hip_stream_sync(None)
    # the residual entries refuse what the old ones refuse, and write nothing
    rcs = [st.inter_qp(cus=None), st.inter_qp(prm=None), st.inter_qp(sy=QC.KNOWN_W - 1), st.intra_qp(modes=None), st.intra_qp(prm=None),
           st.intra_qp(cy=st.ptr("coeff", 0) + 2)]
    assert rcs == [-2] * len(rcs)


def chain_expected(case, start_qp):
    src, pred, cus, modes, lcu_qp = case
    h, w = src[0].shape
    _, full, mapped, last = QC.compose_chain(src, pred, cus, modes, lcu_qp, start_qp, 0, B=O, init=QC.zero_outputs(w, h, 1), many=True)
    deb = QC.backend().deblock_frame(full["rec"][0], full["rec"][1], full["rec"][2], mapped, deblock_params(qp=start_qp, per_cu_qp=1))
    return full, mapped, last, deb


def test_chain_to_deblocking_on_one_stream_and_replayed_from_a_graph(api):
    """residual -> intra -> QP map -> deblocking with per_cu_qp = 1; the graph is replayed after the CONTENTS of lcu_qp, the source and
    the CU map changed, against the CPU composition followed by the reference's deblocking (the oracle's where the reference is not
    built: tests/test_lcu_qp_ref.py holds the two together on this picture)"""
    w, h, start_qp = 200, 136, 31
    first, second = QC.chain_case(w, h, 2000), QC.chain_case(w, h, 2010)
    assert not np.array_equal(first[4], second[4]) and not np.array_equal(first[2].view(np.uint8), second[2].view(np.uint8))
    src, pred, cus, modes, lcu_qp = first
    st = Staged(api, src, pred, cus, modes, lcu_qp, init=QC.zero_outputs(w, h, 1))
    dprm = deblock_params(qp=start_qp, per_cu_qp=1)
    L, s, graph = st.L, st.L.kvz_hip_stream_create(), C.c_void_p()

    def launch():
        check(st.inter_qp(s), "inter_residual_frame_qp")
        check(st.intra_qp(s), "intra_recon_frame_qp")
        check(st.cu_qp(start_qp, 0, s), "cu_qp_frame")
        check(L.kvz_hip_deblock_frame(st.ptr("rec", 0), w, st.ptr("rec", 1), st.ptr("rec", 2), w // 2, w, h, st.ptr("cus"), dprm.ctypes.data, s), "deblock_frame")

    def compare(case, what):
        full, mapped, last, deb = chain_expected(case, start_qp)
        got = st.result()
        for k in range(3):
            np.testing.assert_array_equal(got["rec"][k], deb[k], err_msg="%s: plane %d after deblocking" % (what, k))
            np.testing.assert_array_equal(got["coeff"][k], full["coeff"][k], err_msg="%s: coefficients %d" % (what, k))
        np.testing.assert_array_equal(got["cus"].view(np.uint8), mapped.view(np.uint8), err_msg=what)
        np.testing.assert_array_equal(got["last"], last, err_msg=what)
        np.testing.assert_array_equal(got["cbf_out"], full["cbf_out"], err_msg=what)
        np.testing.assert_array_equal(got["costs"].view(np.uint32), full["costs"].view(np.uint32), err_msg=what)

    try:
        launch()                                                        # four asynchronous calls, nothing between them
        check(L.kvz_hip_stream_sync(s), "sync")
        compare(first, "eager")
        check(L.kvz_hip_graph_begin(s), "graph_begin")
        launch()
        check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        zero = QC.zero_outputs(w, h, 1)
        for n, case in enumerate((second, first)):
            src, pred, cus, modes, lcu_qp = case
            for k in range(3):
                st.upload("src", k, src[k], s)
                st.upload("rec", k, pred[k], s)
                st.upload("coeff", k, zero[0][k], s)
            st.upload("cus", 0, cus, s)
            st.upload("modes", 0, modes, s)
            st.upload("cbf_out", 0, zero[1], s)
            st.upload("costs", 0, zero[2], s)
            st.upload("last", 0, st.host["last"][0], s)
            st.set_lcu_qp(lcu_qp, s)
            check(L.kvz_hip_stream_sync(s), "sync")
            check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            check(L.kvz_hip_stream_sync(s), "sync")
            st.host["src"] = [np.ascontiguousarray(p) for p in src]
            st.host["modes"] = [np.ascontiguousarray(modes)]
            compare(case, "replay %d" % n)
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)

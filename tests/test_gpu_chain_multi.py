"""GPU: the multi-picture entries of the picture chain's residual stages -- kvz_hip_inter_residual_frames and kvz_hip_intra_recon_frames --
against the three committed fixtures (intra_recon.npz, lcu_qp.npz, inter_residual.npz) and against the single-picture _qp entries on a
second staging of the same inputs.  The pictures of one call differ in size (96 x 72 to 256 x 192, so rows and wavefronts run out at
different launches), in chroma format, QP, sign hiding and slice type, and in whether they carry lcu_qp, cbf_out and costs.  One staging
per picture: every array between guard bands, every output poisoned, the QP array at an odd address; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import inter_residual_cases as RC
import intra_recon_cases as XC
import lcu_qp_cases as QC
import oracle_lib as O
import test_gpu_inter_residual as TR
import test_gpu_intra_recon as TX
import test_gpu_lcu_qp as TQ

pytestmark = pytest.mark.gpu

INVALID = -2


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


class Pic:
    """one picture of a fixture: its inputs, the initial contents of its outputs, what the stages leave and which stages it takes"""

    def __init__(self, name, stages, src, pred, cus, modes, lcu_qp, qp, chroma, signhide, slice_is_intra, init, want):
        self.name, self.stages, self.src, self.pred, self.cus, self.modes, self.lcu_qp = name, stages, src, pred, cus, modes, lcu_qp
        self.qp, self.chroma, self.signhide, self.slice_is_intra, self.init, self.want = qp, chroma, signhide, slice_is_intra, init, want
        self.h, self.w = src[0].shape

    def stage(self, A, **content):
        """a staging of its own: test_gpu_lcu_qp.Staged, whose QP array holds zeros where the picture has none (and is not passed)"""
        c = {"src": self.src, "pred": self.pred, "cus": self.cus, "modes": self.modes, "lcu_qp": self.lcu_qp}
        c.update(content)
        lx, ly = QC.lcu_grid(self.w, self.h)
        q = c["lcu_qp"] if c["lcu_qp"] is not None else np.zeros(lx * ly, np.int8)
        return TQ.Staged(A, c["src"], c["pred"], c["cus"], c["modes"], q, self.qp, self.chroma, self.signhide, self.slice_is_intra, init=self.init)

    def untouched(self):
        return {"rec": self.pred, "coeff": self.init[0], "cus": self.cus, "cbf_out": self.init[1], "costs": self.init[2]}


_PICS = {}


def pictures(kind):
    """the pictures of one fixture file, loaded once and never changed"""
    if kind not in _PICS:
        out = []
        if kind == "intra":
            z = np.load(TX.GOLDEN, allow_pickle=False)
            for (name, w, h, chroma, qp, signhide, slice_is_intra) in (p[:7] for p in XC.FIXTURE_PICTURES):
                src, rec, cus, modes, want = XC.load_fixture_case(z, name, chroma)
                out.append(Pic("intra_recon " + name, ("intra",), src, rec, cus, modes, None, qp, chroma, signhide, slice_is_intra,
                               RC.initial_outputs(w, h, chroma), want))
        elif kind == "qp":
            z = np.load(TQ.GOLDEN, allow_pickle=False)
            for (name, w, h, chroma, signhide, slice_is_intra) in (p[:6] for p in QC.FIXTURE_PICTURES):
                src, pred, cus, modes, lcu_qp, want = QC.load_fixture_case(z, name, chroma)
                out.append(Pic("lcu_qp " + name, ("inter", "intra"), src, pred, cus, modes, lcu_qp, QC.PARAMS_QP, chroma, signhide, slice_is_intra,
                               QC.zero_outputs(w, h, chroma), want["full"]))
        else:
            z = np.load(TR.GOLDEN, allow_pickle=False)
            for (name, w, h, chroma, qp, signhide, _) in RC.FIXTURE_PICTURES:
                src, pred, cus, want = RC.load_fixture_case(z, name, chroma)
                out.append(Pic("inter_residual " + name, ("inter",), src, pred, cus, np.zeros(cus.shape + (2,), np.uint8), None, qp, chroma, signhide, 0,
                               RC.initial_outputs(w, h, chroma), want))
        _PICS[kind] = out
    return _PICS[kind]


def record(st, lcu_qp, cbf=True, costs=True):
    """kvz_hip_chain_picture of a staging"""
    from kvazaar_amd import _lib as B
    t, a, p = st.table[0], st.args({}), st.prm[0]
    r = B.ChainPicture()
    r.src = B.RefPicture(int(t["y"]) or None, int(t["u"]) or None, int(t["v"]) or None, int(t["stride_y"]), int(t["stride_c"]), int(t["width"]), int(t["height"]))
    r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c = a["y"], a["u"], a["v"], a["sy"], a["sc"]
    r.cus, r.intra_modes, r.coeff_y, r.coeff_u, r.coeff_v = a["cus"], a["modes"], a["cy"], a["cu"], a["cv"]
    r.cbf_out, r.costs = a["cbf"] if cbf else None, a["costs"] if costs else None
    r.lcu_qp = st.qp_ptr() if lcu_qp else None
    r.params = B.InterResidualParams(int(p["qp"]), int(p["slice_is_intra"]), int(p["signhide"]), int(p["scaling_list"]), int(p["chroma"]), 0)
    return r


class Batch:
    """stagings and records of one call"""

    def __init__(self, A, pics, cbf=None, costs=None):
        from kvazaar_amd import _lib as B
        self.B, self.pics = B, list(pics)
        self.st = [p.stage(A) for p in self.pics]
        n = len(self.pics)
        self.cbf, self.costs = cbf or [True] * n, costs or [True] * n
        self.records = (B.ChainPicture * max(n, 1))(*[record(st, p.lcu_qp is not None, self.cbf[i], self.costs[i])
                                                     for i, (st, p) in enumerate(zip(self.st, self.pics))])
        self.L = B.load()

    def subset(self, stage):
        keep = [i for i, p in enumerate(self.pics) if stage in p.stages]
        return (self.B.ChainPicture * max(len(keep), 1))(*[self.records[i] for i in keep]), len(keep)

    def run(self, stream=None):
        """the inter stage of the pictures that take it, then the intra stage of those that take it: two calls"""
        recs, n = self.subset("inter")
        self.B.check(self.L.kvz_hip_inter_residual_frames(recs, n, stream), "inter_residual_frames")
        recs, n = self.subset("intra")
        self.B.check(self.L.kvz_hip_intra_recon_frames(recs, n, stream), "intra_recon_frames")

    def sync(self, stream=None):
        self.B.check(self.L.kvz_hip_stream_sync(stream), "sync")

    def compare(self, what):
        for p, st in zip(self.pics, self.st):
            XC.assert_outputs_equal(st.result(), p.want, "%s: %s" % (what, p.name), p.chroma)


def run_batch(A, pics, what):
    b = Batch(A, pics)
    b.run()
    b.sync()
    b.compare(what)
    return b


def test_all_four_intra_fixture_pictures_in_one_call(api):
    """200 x 136 ragged, 256 x 192 all-intra in an I slice, 128 x 128 4:0:0 and 128 x 64: rows and wavefronts of the smaller pictures run
    out, a 4:0:0 picture stands beside 4:2:0 ones, and QP, signhide and slice type are each picture's own"""
    pics = pictures("intra")
    assert len(pics) == 4 and {(p.w, p.h) for p in pics} == {(200, 136), (256, 192), (128, 128), (128, 64)}
    assert {p.chroma for p in pics} == {0, 1} and {p.qp for p in pics} == {27, 37} and {p.signhide for p in pics} == {0, 1} and {p.slice_is_intra for p in pics} == {0, 1}
    b = Batch(api, pics)
    recs, n = b.subset("inter")
    assert n == 0 and b.L.kvz_hip_inter_residual_frames(recs, 0, None) == 0
    b.run()
    b.sync()
    b.compare("one call")


def test_lcu_qp_fixture_through_both_entries_then_mixed_with_pictures_without_an_array(api):
    qp = pictures("qp")
    assert len(qp) == 3 and {p.chroma for p in qp} == {0, 1}
    run_batch(api, qp, "three pictures with lcu_qp")
    # lcu_qp present and absent in one call of either entry: the inter call takes the lcu_qp pictures and the inter_residual ones, the
    # intra call the lcu_qp pictures and two of intra_recon
    x, r = pictures("intra"), pictures("inter")
    mix = [qp[0], r[0], x[0], qp[1], r[1], qp[2], x[2], r[2]]
    b = Batch(api, mix)
    for stage, count in (("inter", 6), ("intra", 5)):
        recs, n = b.subset(stage)
        assert n == count and {bool(recs[i].lcu_qp) for i in range(n)} == {True, False}
    b.run()
    b.sync()
    b.compare("lcu_qp present and absent")


def test_order_and_count(api):
    pics = pictures("intra")
    run_batch(api, pics[::-1], "reversed")
    for p in pics + pictures("qp"):
        run_batch(api, [p], "alone")
    sixteen = (pics * 4)[:16]
    b = run_batch(api, sixteen, "sixteen")
    assert len(b.st) == 16 and len({st.ptr("rec", 0) for st in b.st}) == 16
    both = (pictures("qp") * 6)[:16]
    run_batch(api, both, "sixteen through both entries")


def test_equals_the_single_picture_entries_with_optional_outputs_given_and_null(api):
    """the rule itself: per picture the bytes kvz_hip_inter_residual_frame_qp / kvz_hip_intra_recon_frame_qp leave on a second staging, with
    cbf_out and costs NULL for some pictures and given for others, and lcu_qp NULL for some"""
    qp, x = pictures("qp"), pictures("intra")
    pics = [qp[0], x[1], qp[1], qp[2], x[3]]
    cbf, costs = [True, True, False, False, True], [True, False, True, False, False]
    b = Batch(api, pics, cbf, costs)
    b.run()
    b.sync()
    for i, (p, st) in enumerate(zip(pics, b.st)):
        single = p.stage(api)
        over = {}
        if p.lcu_qp is None:
            over["lcu_qp"] = None
        if not cbf[i]:
            over["cbf"] = None
        if not costs[i]:
            over["costs"] = None
        if "inter" in p.stages:
            TQ.check(single.inter_qp(**over), "inter_residual_frame_qp")
        TQ.check(single.intra_qp(**over), "intra_recon_frame_qp")
        TQ.check(single.L.kvz_hip_stream_sync(None), "sync")
        want, got = single.result(), st.result()
        XC.assert_outputs_equal(got, want, p.name, p.chroma)
        if not cbf[i]:
            assert (got["cbf_out"] == p.init[1]).all(), "cbf_out was written though NULL was passed"
        if not costs[i]:
            np.testing.assert_array_equal(got["costs"].view(np.uint32), p.init[2].view(np.uint32), err_msg="costs were written though NULL was passed")
        if cbf[i] and costs[i]:
            XC.assert_outputs_equal(got, p.want, p.name + " against the fixture", p.chroma)


def test_refusals_write_nothing_and_name_the_record(api):
    pics = pictures("intra")
    b = Batch(api, pics)
    L, n = b.L, len(pics)
    good = b.records[2]

    def bad(**fields):
        recs = (b.B.ChainPicture * n)(*[b.records[i] for i in range(n)])
        for k, v in fields.items():
            if k == "width":
                recs[2].src.width = v
            elif k == "scaling_list":
                recs[2].params.scaling_list = v
            else:
                setattr(recs[2], k, v)
        return recs

    cases = [bad(coeff_y=None), bad(width=pics[2].w - 4), bad(scaling_list=1), bad(rec_y=b.records[0].rec_y)]
    assert good.coeff_y and good.src.width % 8 == 0 and good.params.scaling_list == 0 and good.rec_y != b.records[0].rec_y
    for entry in (L.kvz_hip_inter_residual_frames, L.kvz_hip_intra_recon_frames):
        for recs in cases:
            assert entry(recs, n, None) == INVALID
            assert b"picture 2" in L.kvz_hip_last_error(), L.kvz_hip_last_error()
        assert entry(b.records, 0, None) == 0 and entry(None, 0, None) == 0
        assert entry(b.records, 17, None) == INVALID and entry(b.records, -1, None) == INVALID and entry(None, n, None) == INVALID
    b.sync()
    for p, st in zip(pics, b.st):
        XC.assert_outputs_equal(st.result(), p.untouched(), p.name + " after refused calls", p.chroma)
    assert L.kvz_hip_abi_version() == 4
    # and the same records are accepted as they stand
    b.run()
    b.sync()
    b.compare("after the refusals")


def test_both_calls_replayed_from_a_graph_after_the_contents_changed(api):
    """a linear capture of the two calls on one stream; the replay runs on a second seed's inputs in two of the three pictures, against the
    composition of the reference's own functions (lcu_qp_cases.compose_chain over the oracle)"""
    pics = pictures("qp")
    b = Batch(api, pics)
    L, s, graph = b.L, b.L.kvz_hip_stream_create(), C.c_void_p()
    try:
        b.B.check(L.kvz_hip_graph_begin(s), "graph_begin")
        b.run(s)
        b.B.check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        b.B.check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
        b.sync(s)
        b.compare("first launch")
        want = []
        for i, (p, st) in enumerate(zip(pics, b.st)):
            if i == 2:
                src, pred, cus, modes, lcu_qp = p.src, p.pred, p.cus, p.modes, p.lcu_qp          # this one runs again on what it had
                want.append(p.want)
            else:
                src, pred, cus, modes, lcu_qp = QC.chain_case(p.w, p.h, 3000 + i, p.chroma)
                want.append(QC.compose_chain(src, pred, cus, modes, lcu_qp, 30, 0, p.chroma, p.signhide, p.slice_is_intra, B=O, init=p.init, many=True)[1])
            for k in range(3 if p.chroma else 1):
                st.upload("src", k, src[k], s)
                st.upload("rec", k, pred[k], s)
                st.upload("coeff", k, p.init[0][k], s)
            st.upload("cus", 0, cus, s)
            st.upload("modes", 0, modes, s)
            st.upload("cbf_out", 0, p.init[1], s)
            st.upload("costs", 0, p.init[2], s)
            st.set_lcu_qp(lcu_qp, s)
            st.host["src"] = [np.ascontiguousarray(a) for a in src[:3 if p.chroma else 1]]
            st.host["modes"] = [np.ascontiguousarray(modes)]
        b.sync(s)
        b.B.check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
        b.sync(s)
        for p, st, w in zip(pics, b.st, want):
            XC.assert_outputs_equal(st.result(), w, "replay: " + p.name, p.chroma)
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


def test_numpy_conveniences_on_one_batch(api):
    pics = pictures("qp")
    mid = api.inter_residual_frames([dict(src=p.src, pred=p.pred, cus=p.cus, qp=p.qp, chroma=p.chroma, slice_is_intra=p.slice_is_intra, signhide=p.signhide,
                                          coeff=p.init[0], cbf_out=p.init[1], costs=p.init[2], lcu_qp=p.lcu_qp) for p in pics])
    full = api.intra_recon_frames([dict(src=p.src, rec=m["rec"], cus=m["cus"], modes=p.modes, qp=p.qp, chroma=p.chroma, signhide=p.signhide,
                                        slice_is_intra=p.slice_is_intra, coeff=m["coeff"], cbf_out=m["cbf_out"], costs=m["costs"], lcu_qp=p.lcu_qp)
                                   for p, m in zip(pics, mid)])
    assert len(mid) == len(full) == len(pics)
    for p, got in zip(pics, full):
        XC.assert_outputs_equal(got, p.want, p.name + " convenience", p.chroma)
    # without an array: the intra_recon pictures, each with its own QP
    x = pictures("intra")
    got = api.intra_recon_frames([dict(src=p.src, rec=p.pred, cus=p.cus, modes=p.modes, qp=p.qp, chroma=p.chroma, signhide=p.signhide,
                                       slice_is_intra=p.slice_is_intra, coeff=p.init[0], cbf_out=p.init[1], costs=p.init[2]) for p in x])
    for p, g in zip(x, got):
        XC.assert_outputs_equal(g, p.want, p.name + " convenience", p.chroma)
    assert api.inter_residual_frames([]) == [] and api.intra_recon_frames([]) == []

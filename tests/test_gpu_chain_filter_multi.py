"""GPU: the multi-picture entries behind the residual stages -- kvz_hip_cu_qp_frames, kvz_hip_deblock_frames, kvz_hip_sao_stats_frames
and kvz_hip_sao_frames -- against the committed fixtures (tile_chain.npz, lcu_qp.npz, sao_frame.npz) and against the single-picture
entries (kvz_hip_cu_qp_frame_tiles, kvz_hip_deblock_frame_tiles, kvz_hip_sao_stats_frame, kvz_hip_sao_frame_tiles) on a second staging of
the same inputs.  The pictures of one call differ in size (8 x 8 to 256 x 128: the workgroups of a small picture run out while a large
one's go on), in their tile grid (tiled beside untiled), in chroma format, in chain_rows and in their deblock parameters.  One staging
per picture (test_gpu_tile_chain.Staged, test_gpu_sao_frame.Staged): every array between guard bands, every output poisoned, the QP
array at an odd address; every comparison is exact.  deblock.npz is not used: its loader gives block lists, not the arguments of a
picture entry.  After a call or a synchronisation that reports a runtime error no further test starts anything on the device."""
import ctypes as C
import faulthandler
import sys

import numpy as np
import pytest

import lcu_qp_cases as QC
import sao_frame_cases as SC
import test_gpu_inter_residual as TR
import test_gpu_lcu_qp as QL
import test_gpu_sao_frame as SF
import test_gpu_tile_chain as TT
import tile_chain_cases as TC

pytestmark = pytest.mark.gpu

INVALID = -2
TEST_LIMIT_S = 60                                                     # every test takes a few seconds at the most
FAULTS = []
STAGES = ("qp", "deblock", "stats", "sao")
ENTRIES = {"qp": "kvz_hip_cu_qp_frames", "deblock": "kvz_hip_deblock_frames", "stats": "kvz_hip_sao_stats_frames", "sao": "kvz_hip_sao_frames"}


def check(rc, what):
    try:
        QL.check(rc, what)
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


# ---------------------------------------------------------------- the pictures: their contents before the QP map, loaded once
_STATES = {}


def states():
    """{name: state}.  A "chain" state is a picture after the intra stage (all four stages); a "sao" state is a picture of sao_frame.npz
    (the two SAO stages).  Never changed: changed() makes copies"""
    if _STATES:
        return _STATES
    z = np.load(TT.GOLDEN, allow_pickle=False)
    for pic in TC.FIXTURE_PICTURES:
        case, want = TC.load_fixture_case(z, pic)
        _STATES["tile " + pic[0]] = dict(case, kind="chain", pred=want["full"]["rec"], cus=want["full"]["cus"], cbf=want["full"]["cbf_out"], tiled=True,
                                         want=want)
    z = np.load(TT.LCU_QP_GOLDEN, allow_pickle=False)
    for pic in QC.FIXTURE_PICTURES:
        name, w, h, chroma, signhide, slice_is_intra, seed, share, start_qp, _ = pic
        src, pred, cus, modes, lcu_qp, want = QC.load_fixture_case(z, name, chroma)
        luma, chro = TC.sao_records(w, h, 5 + seed, None, None)
        col_bd, row_bd = TC.one_tile(w, h)
        _STATES["qp " + name] = {"kind": "chain", "name": name, "width": w, "height": h, "chroma": chroma, "signhide": signhide, "slice_is_intra": slice_is_intra,
                                 "start_qp": start_qp, "col_bd": list(col_bd), "row_bd": list(row_bd), "src": src, "pred": want["full"]["rec"],
                                 "cus": want["full"]["cus"], "modes": modes, "lcu_qp": lcu_qp, "sao_luma": luma, "sao_chroma": chro if chroma else None,
                                 "cbf": want["full"]["cbf_out"], "tiled": False, "want": want}
    z = np.load(SF.GOLDEN, allow_pickle=False)
    for name, w, h, chroma, seed in SC.FIXTURE_PICTURES:
        src, rec, luma, chro, want = SC.load_fixture_case(z, name, chroma)
        _STATES["sao " + name] = {"kind": "sao", "name": name, "width": w, "height": h, "chroma": chroma, "src": src, "pred": rec, "sao_luma": luma,
                                  "sao_chroma": chro, "want": want}
    return _STATES


def changed(state, seed):
    """the same picture with other contents in every array a stage reads; the map keeps its tree"""
    g = np.random.default_rng(seed)
    noise = lambda p: None if p is None else np.clip(p.astype(np.int32) + g.integers(-9, 10, p.shape), 0, 255).astype(np.uint8)
    new = dict(state, src=tuple(noise(p) for p in state["src"]), pred=tuple(noise(p) for p in state["pred"]), want=None)
    new["sao_luma"] = np.roll(np.asarray(state["sao_luma"]).reshape(-1, 14), 1, axis=0)
    if state["sao_chroma"] is not None:
        new["sao_chroma"] = np.roll(np.asarray(state["sao_chroma"]).reshape(-1, 14), 1, axis=0)
    if state["kind"] == "chain":
        new["cbf"] = (state["cbf"] != 0).astype(np.uint8) ^ (g.random(state["cbf"].shape) < 0.2).astype(np.uint8)
        new["lcu_qp"] = g.integers(0, 52, len(state["lcu_qp"])).astype(np.int8)
        new["cus"] = np.array(state["cus"])
        new["cus"]["qp"] = 0x2A
    return new


class Pic:
    """one picture of a call: its staging, its record, the single-picture entries with its fields, and what the stages leave"""

    def __init__(self, A, state, chain_rows=0, prm=None, cands=True):
        from kvazaar_amd import _lib as B
        self.A, self.B, self.state, self.kind, self.chain_rows, self.with_cands = A, B, state, state["kind"], chain_rows, cands
        self.w, self.h, self.chroma = state["width"], state["height"], state["chroma"]
        self.stages = STAGES if self.kind == "chain" else STAGES[2:]
        n = 3 if self.chroma else 1
        if self.kind == "chain":
            zero = QC.zero_outputs(self.w, self.h, self.chroma)
            self.st = st = TT.Staged(A, state, init=(zero[0], np.ascontiguousarray(state["cbf"]), zero[2]))
            words = lambda m: np.full(m, SC.POISON_WORD, np.uint32).view(np.int32)
            lcus = A.lcu_count(self.w, self.h)
            st.host["stats"], st.host["cands"] = [words(n * lcus * 104)], [words(n * lcus * 30)]
            for k in ("stats", "cands"):
                st.dev[k] = [st._up(st.host[k][0])]
            if prm is not None:
                st.dprm = prm
            self.grid = st.grid if state["tiled"] else None
        else:
            # planes inside larger buffers, every stride its own (the largest picture only: the others stay compact)
            planes = lambda key, fill: [SF.embed(p, p.shape[1] + (12 if k == 0 else 8), 4 * (k > 0), k + 1, fill) for k, p in enumerate(state[key][:n])]
            big = self.w >= 200
            dst = [SF.poisoned(v) for v in planes("pred", 0)] if big else None
            self.st = SF.Staged(A, planes("src", 0x11) if big else state["src"], planes("pred", 0x22) if big else state["pred"], state["sao_luma"],
                                state["sao_chroma"], self.chroma, dst=dst)
            self.grid = None
        self.L = self.st.L

    def record(self):
        B, st, r = self.B, self.st, self.B.FilterPicture()
        r.width, r.height, r.chroma = self.w, self.h, self.chroma
        r.deblock.chroma = self.chroma
        ch = self.chroma
        if self.kind == "chain":
            r.src = B.RefPicture(st.ptr("src", 0), st.ptr("src", 1), st.ptr("src", 2), self.w, self.w // 2 if ch else 0, self.w, self.h)
            r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c = st.ptr("rec", 0), st.ptr("rec", 1), st.ptr("rec", 2), self.w, self.w // 2 if ch else 0
            r.dst_y, r.dst_u, r.dst_v, r.dst_stride_y, r.dst_stride_c = st.ptr("dst", 0), st.ptr("dst", 1), st.ptr("dst", 2), self.w, self.w // 2 if ch else 0
            r.cus, r.cbf, r.lcu_qp, r.lcu_last_qp = st.ptr("cus"), st.ptr("cbf_out"), st.qp_ptr(), st.ptr("last")
            r.sao_luma, r.sao_chroma = st.ptr("sao", 0), st.ptr("sao", 1)
            r.deblock = B.DeblockParams.from_buffer_copy(np.ascontiguousarray(st.dprm).tobytes())
            r.cu_qp = B.CuQpTilesParams(st.start_qp, self.chain_rows)
            if self.grid is not None:
                r.grid = C.cast(self.grid.ctypes.data, C.POINTER(B.TileGrid))
        else:
            r.src = B.RefPicture(st.ptr("src", 0), st.ptr("src", 1), st.ptr("src", 2), st.src[0].stride, st.src[1].stride if ch else 0, self.w, self.h)
            r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c = st.ptr("rec", 0), st.ptr("rec", 1), st.ptr("rec", 2), st.rec[0].stride, st.rec[1].stride if ch else 0
            r.dst_y, r.dst_u, r.dst_v = st.ptr("dst", 0), st.ptr("dst", 1), st.ptr("dst", 2)
            r.dst_stride_y, r.dst_stride_c = st.dst[0].stride, st.dst[1].stride if ch else 0
            r.sao_luma, r.sao_chroma = st.ptr("luma"), st.ptr("chro")
        r.stats, r.cands = st.ptr("stats"), st.ptr("cands") if self.with_cands else None
        return r

    def single(self, stage, stream=None):
        """the single-picture entry of the stage with this picture's fields"""
        st = self.st
        g = {} if self.grid is not None else {"grid": None}
        if self.kind == "sao":
            over = {} if self.with_cands else {"cands": None}
            check(st.stats_call(stream, **over) if stage == "stats" else st.frame_call(stream), "single " + stage)
        elif stage == "qp":
            check(st.cu_qp_tiles(self.chain_rows, stream, **g), "cu_qp_frame_tiles")
        elif stage == "deblock":
            check(st.deblock_tiles(stream, **g), "deblock_frame_tiles")
        elif stage == "sao":
            check(st.sao_tiles(stream, **g), "sao_frame_tiles")
        else:
            check(self.L.kvz_hip_sao_stats_frame(st.table.ctypes.data, st.ptr("rec", 0), self.w, st.ptr("rec", 1), st.ptr("rec", 2),
                                                 self.w // 2 if self.chroma else 0, self.chroma, st.ptr("stats"),
                                                 st.ptr("cands") if self.with_cands else None, stream), "sao_stats_frame")

    def load(self, state, stream=None):
        """other contents into every device array, outputs poisoned again"""
        st, n = self.st, 3 if self.chroma else 1
        for k in range(n):
            if self.kind == "chain":
                st.upload("src", k, state["src"][k], stream)
                st.upload("rec", k, state["pred"][k], stream)
                st.host["src"][k] = np.ascontiguousarray(state["src"][k])
            else:
                for kind, key in (("src", "src"), ("rec", "pred")):
                    buf = np.array(st.host[kind][k])
                    getattr(st, kind)[k].crop(buf)[:] = state[key][k]
                    st.upload(kind, k, buf, stream)
            st.upload("dst", k, np.full(st.host["dst"][k].shape, TT.POISON_DST if self.kind == "chain" else SC.POISON_PIXEL, np.uint8), stream)
        luma, chro = np.ascontiguousarray(state["sao_luma"], dtype=np.int32).reshape(-1, 14), state["sao_chroma"]
        if self.kind == "chain":
            st.upload("sao", 0, luma, stream)
            st.host["sao"][0] = luma
            if chro is not None:
                st.host["sao"][1] = np.ascontiguousarray(chro, dtype=np.int32).reshape(-1, 14)
                st.upload("sao", 1, st.host["sao"][1], stream)
            st.upload("cus", 0, state["cus"], stream)
            st.upload("cbf_out", 0, state["cbf"], stream)
            st.upload("last", 0, st.host["last"][0], stream)
            st.set_lcu_qp(state["lcu_qp"], stream)
        else:
            st.upload("luma", 0, luma, stream)
            if chro is not None:
                st.upload("chro", 0, np.ascontiguousarray(chro, dtype=np.int32).reshape(-1, 14), stream)
        for k in ("stats", "cands"):
            st.upload(k, 0, np.full(st.host[k][0].shape, SC.POISON_WORD, np.uint32).view(np.int32), stream)

    def result(self):
        """every output, as arrays; asserts every guard band and that no input changed"""
        st = self.st
        out = st.result()
        if self.kind == "chain":
            inner = lambda kind: st.raw(kind, 0)[TR.GUARD:-TR.GUARD].view(np.int32)
            return {"rec": out["rec"], "dst": out["dst"], "cus": out["cus"].view(np.uint8), "last": out["last"], "cbf": out["cbf_out"],
                    "stats": inner("stats"), "cands": inner("cands")}
        return {"dst": tuple(out["dst_buf"]) + (None,) * (3 - len(out["dst_buf"])), "stats": out["stats"].view(np.int32), "cands": out["cands"].view(np.int32)}


def same(got, want, what):
    assert got.keys() == want.keys()
    for key in got:
        for k, (a, b) in enumerate(zip(got[key], want[key]) if isinstance(got[key], tuple) else [(got[key], want[key])]):
            if a is not None or b is not None:
                np.testing.assert_array_equal(a, b, err_msg="%s: %s %d" % (what, key, k))


class Batch:
    def __init__(self, pics):
        self.pics = list(pics)
        self.B, self.L = pics[0].B, pics[0].L
        self.records = [p.record() for p in self.pics]

    def table(self, stage):
        keep = [r for p, r in zip(self.pics, self.records) if stage in p.stages]
        return (self.B.FilterPicture * max(len(keep), 1))(*keep), len(keep)

    def call(self, stage, stream=None):
        recs, n = self.table(stage)
        check(getattr(self.L, ENTRIES[stage])(recs, n, stream), ENTRIES[stage])

    def run(self, stream=None, stages=STAGES):
        for stage in stages:
            self.call(stage, stream)

    def singles(self, stream=None, stages=STAGES):
        for stage in stages:
            for p in self.pics:
                if stage in p.stages:
                    p.single(stage, stream)

    def sync(self, stream=None):
        check(self.L.kvz_hip_stream_sync(stream), "sync")

    def results(self):
        return [p.result() for p in self.pics]


def assert_rule(api, specs, what):
    """the multi entries on one staging against the single-picture entries on a second one; specs: (state name, Pic keywords)"""
    S = states()
    multi, single = Batch([Pic(api, S[n], **kw) for n, kw in specs]), Batch([Pic(api, S[n], **kw) for n, kw in specs])
    multi.run()
    multi.sync()
    single.singles()
    single.sync()
    for (n, kw), got, want, p in zip(specs, multi.results(), single.results(), multi.pics):
        same(got, want, "%s: %s %s" % (what, n, kw))
        assert (got["stats"] != SC.POISON_WORD).all() and (p.with_cands or (got["cands"] == SC.POISON_WORD).all())
        if p.kind == "chain":
            assert (got["last"] != QL.POISON_LAST).all() and (got["dst"][0] != TT.POISON_DST).any()
    return multi


# ---------------------------------------------------------------- 1. the fixtures, one call per stage
def test_fixture_pictures_in_one_call_per_stage(api):
    S = states()
    names = ["tile " + p[0] for p in TC.FIXTURE_PICTURES]
    assert [(S[n]["width"], S[n]["height"], S[n]["chroma"]) for n in names] == [(200, 136, 1), (192, 64, 1), (96, 72, 0)]
    assert S[names[0]]["col_bd"] == [0, 1, 4] and S[names[0]]["row_bd"] == [0, 2, 3] and len(S[names[1]]["col_bd"]) == 4
    # chain_rows 0 and 1 in the same call, and the untiled pictures of lcu_qp.npz beside the tiled ones
    qp_names = names + ["qp " + p[0] for p in QC.FIXTURE_PICTURES]
    for rows in (1, 0):
        pics = [Pic(api, S[n], chain_rows=rows ^ (i & 1)) for i, n in enumerate(qp_names)]
        b = Batch(pics)
        b.call("qp")
        b.sync()
        for p, n, got in zip(pics, qp_names, b.results()):
            want = S[n]["want"]
            np.testing.assert_array_equal(got["cus"], want["cus_qp_rows" if p.chain_rows else "cus_qp"].view(np.uint8), err_msg="%s chain_rows %d" % (n, p.chain_rows))
            np.testing.assert_array_equal(got["last"], want["last_rows" if p.chain_rows else "last"], err_msg="%s chain_rows %d" % (n, p.chain_rows))
    # the three tiled pictures on through deblocking and SAO: the QP map with chain_rows 0 is what the fixture's deblocking read
    b = Batch([Pic(api, S[n]) for n in names])
    b.run()
    b.sync()
    for n, got in zip(names, b.results()):
        want = S[n]["want"]
        TT.assert_planes(got["rec"], want["deb"], n + " after deblocking")
        TT.assert_planes(got["dst"], want["sao"], n + " after SAO")
        np.testing.assert_array_equal(got["cus"], want["cus_qp"].view(np.uint8), err_msg=n + ": the map after the chain")
        assert (got["stats"] != SC.POISON_WORD).all() and (got["cands"] != SC.POISON_WORD).all()


def test_sao_fixture_pictures_in_one_call(api):
    S = states()
    names = ["sao " + p[0] for p in SC.FIXTURE_PICTURES]
    assert [(S[n]["width"], S[n]["height"]) for n in names] == [(200, 136), (136, 72), (64, 64), (8, 8)]     # 8 x 8 beside a grid sized for 200 x 136
    pics = [Pic(api, S[n]) for n in names]
    b = Batch(pics)
    b.run(stages=("stats", "sao"))
    b.sync()
    for p, n in zip(pics, names):
        SF.assert_equal(p.st.result(), S[n]["want"], n, p.chroma)


# ---------------------------------------------------------------- 2. against the single-picture entries on a second staging
MIXED = [("tile ragged", {}), ("qp mono", {"chain_rows": 1}), ("sao tiny", {}), ("tile columns", {"chain_rows": 1}), ("qp coarse", {}),
         ("sao ragged", {"cands": False}), ("tile mono", {}), ("qp ragged", {"chain_rows": 1}), ("sao mono", {})]


def test_every_output_is_the_single_picture_entries_byte_for_byte(api):
    assert_rule(api, MIXED, "mixed")
    assert_rule(api, [MIXED[i] for i in (6, 2, 8, 0, 4, 7, 1, 5, 3)], "permuted")
    # every field of deblock may differ from picture to picture
    other = TC.deblock_params(qp=22, beta=2, tc=-3, per_cu_qp=0, slice_is_b=1, chroma=1)
    assert_rule(api, [("tile ragged", {"prm": other}), ("qp ragged", {}), ("qp coarse", {"prm": other, "chain_rows": 1})], "deblock parameters")


@pytest.mark.parametrize("spec", [MIXED[0], MIXED[1], MIXED[2]], ids=["tiled", "untiled-mono", "tiny"])
def test_one_picture(api, spec):
    assert_rule(api, [spec], "one picture")


def test_sixteen_pictures(api):
    specs = [MIXED[i % len(MIXED)] for i in range(16)]
    b = assert_rule(api, specs, "sixteen")
    assert b.table("sao")[1] == 16 and b.table("qp")[1] == 11


# ---------------------------------------------------------------- 3. a picture sees nothing of another
def test_a_change_in_one_picture_leaves_the_others_bit_identical(api):
    S = states()
    specs = [("tile ragged", {}), ("qp coarse", {"chain_rows": 1}), ("tile mono", {}), ("sao ragged", {})]
    for victim in (1, 3):
        outs = []
        for change in (False, True):
            pics = [Pic(api, changed(S[n], 900 + i) if change and i == victim else S[n], **kw) for i, (n, kw) in enumerate(specs)]
            b = Batch(pics)
            b.run()
            b.sync()
            outs.append(b.results())
        for i, (n, kw) in enumerate(specs):
            if i != victim:
                same(outs[1][i], outs[0][i], "picture %d beside a changed picture %d" % (i, victim))
        assert any((a != b_).any() for a, b_ in zip(outs[0][victim]["dst"], outs[1][victim]["dst"]) if a is not None)
        alone = Pic(api, changed(S[specs[victim][0]], 900 + victim), **specs[victim][1])
        Batch([alone]).singles()
        check(alone.L.kvz_hip_stream_sync(None), "sync")
        same(outs[1][victim], alone.result(), "the changed picture")


# ---------------------------------------------------------------- 4. the four calls on one stream, eager and replayed
def test_four_calls_on_one_stream_and_replayed_from_a_graph_after_the_contents_changed(api):
    S = states()
    specs = [("tile ragged", {}), ("qp mono", {"chain_rows": 1}), ("tile columns", {}), ("qp coarse", {})]
    b = Batch([Pic(api, S[n], **kw) for n, kw in specs])
    L, s, graph = b.L, b.L.kvz_hip_stream_create(), C.c_void_p()
    try:
        check(L.kvz_hip_graph_begin(s), "graph_begin")
        b.run(s)                                                        # QP map -> deblocking -> statistics -> SAO, nothing between them
        check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        for round_, seed in enumerate((None, 4100, 4200)):
            new = [S[n] if seed is None else changed(S[n], seed + i) for i, (n, kw) in enumerate(specs)]
            for p, state in zip(b.pics, new):
                p.load(state, s)
            b.sync(s)
            check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            b.sync(s)
            eager = Batch([Pic(api, state, **kw) for state, (n, kw) in zip(new, specs)])
            eager.run()
            eager.sync()
            for i, (got, want) in enumerate(zip(b.results(), eager.results())):
                same(got, want, "replay %d, picture %d" % (round_, i))
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


# ---------------------------------------------------------------- 5. what the entries refuse
def wide_state(i):
    """1024 x 64, 4:0:0, sixteen tile columns: 16 + 1 + 2 = 19 boundaries of the pool"""
    w, h = 1024, 64
    g = np.random.default_rng(50 + i)
    plane = g.integers(0, 256, (h, w), dtype=np.uint8)
    luma, _ = TC.sao_records(w, h, 7, None, None)
    return {"kind": "chain", "name": "wide", "width": w, "height": h, "chroma": 0, "signhide": 0, "slice_is_intra": 0, "start_qp": 30,
            "col_bd": list(range(17)), "row_bd": [0, 1], "src": (plane, None, None), "pred": (plane, None, None), "cus": np.zeros((h // 4, w // 4), TC.CU_INFO),
            "modes": np.zeros((h // 4, w // 4, 2), np.uint8), "lcu_qp": np.full(16, 30, np.int8), "sao_luma": luma, "sao_chroma": None,
            "cbf": np.zeros((h // 4, w // 4), np.uint8), "tiled": True, "want": None}


def test_refusals_write_nothing_and_name_the_record(api):
    S = states()
    specs = [("tile columns", {}), ("qp coarse", {}), ("tile ragged", {})]
    pics = [Pic(api, S[n], **kw) for n, kw in specs]
    b = Batch(pics)
    L, B = b.L, b.B
    assert (pics[-1].w, pics[-1].h) == (200, 136)
    before = b.results()
    last = len(pics) - 1
    w = pics[last].w

    def refused(stage, edit, n=None, table=True, where=last):
        recs, count = b.table(stage)
        keep = edit(recs) if edit else None
        rc = getattr(L, ENTRIES[stage])(recs if table else None, count if n is None else n, None)
        assert rc == INVALID, (stage, rc)
        msg = L.kvz_hip_last_error().decode()
        assert ENTRIES[stage] in msg, msg
        if edit:
            assert "picture %d" % where in msg, msg
        return keep

    def setter(field, value, i=last):
        def edit(recs):
            obj, names = recs[i], field.split(".")
            for name in names[:-1]:
                obj = getattr(obj, name)
            setattr(obj, names[-1], value(recs) if callable(value) else value)
        return edit

    def grid_edit(g):
        def edit(recs):
            recs[last].grid = C.cast(g.ctypes.data, C.POINTER(B.TileGrid))
            return g
        return edit

    for stage in STAGES:
        for n in (17, -1):
            refused(stage, None, n=n)
        refused(stage, None, table=False)
        assert getattr(L, ENTRIES[stage])(None, 0, None) == 0                       # no pictures: a no-op
        refused(stage, setter("deblock.chroma", 0))
        refused(stage, setter("width", w - 4))
        refused(stage, setter("height", 4))
    for stage, fields in (("qp", ("cus", "cbf", "lcu_qp", "lcu_last_qp")), ("deblock", ("rec_y", "cus", "rec_u")), ("stats", ("stats", "rec_y", "src.y", "src.v")),
                          ("sao", ("sao_luma", "sao_chroma", "rec_y", "dst_y", "dst_v"))):
        for f in fields:
            refused(stage, setter(f, None))
    cus_plus_2 = lambda recs: recs[last].cus + 2
    refused("qp", setter("cus", cus_plus_2))
    refused("deblock", setter("cus", cus_plus_2))
    refused("deblock", setter("rec_y", lambda recs: recs[last].rec_y + 1))
    refused("stats", setter("stats", lambda recs: recs[last].stats + 2))
    refused("stats", setter("cands", lambda recs: recs[last].cands + 1))
    refused("stats", setter("src.width", w + 8))
    refused("sao", setter("sao_luma", lambda recs: recs[last].sao_luma + 2))
    for stage, f in (("deblock", "stride_y"), ("stats", "stride_y"), ("stats", "src.stride_y"), ("sao", "stride_y"), ("sao", "dst_stride_y"), ("sao", "stride_c")):
        refused(stage, setter(f, (w if f[-1] == "y" else w // 2) - 4))
    refused("sao", setter("dst_y", lambda recs: recs[last].rec_y))
    refused("sao", setter("dst_u", lambda recs: recs[last].rec_u))
    # an output base shared with an earlier record
    refused("qp", setter("cus", lambda recs: recs[0].cus))
    refused("qp", setter("lcu_last_qp", lambda recs: recs[1].lcu_last_qp))
    refused("deblock", setter("rec_y", lambda recs: recs[0].rec_y))
    refused("stats", setter("stats", lambda recs: recs[1].stats))
    refused("sao", setter("dst_y", lambda recs: recs[0].dst_y))
    for stage in ("qp", "deblock", "sao"):
        for what, g in TT.bad_grids(api, w, pics[last].h):
            refused(stage, grid_edit(g))
    for value in (-1, 52):
        refused("qp", setter("cu_qp.start_qp", value))
    for value in (2, -1):
        refused("qp", setter("cu_qp.chain_rows", value))
    # the offending record in the middle is named too
    refused("deblock", setter("cus", None, 1), where=1)
    b.sync()
    for i, (got, want) in enumerate(zip(b.results(), before)):
        same(got, want, "after the refusals, picture %d" % i)
        assert (got["last"] == QL.POISON_LAST).all() and (got["dst"][0] == TT.POISON_DST).all() and (got["stats"] == SC.POISON_WORD).all()
    assert L.kvz_hip_abi_version() == 4


def test_pool_overflow_is_a_refusal_that_names_the_record(api):
    from kvazaar_amd import _lib as B
    assert B.CHAIN_TILE_BOUNDS == 256
    pics = [Pic(api, wide_state(i)) for i in range(14)]                 # 13 x 19 = 247 boundaries fit, the fourteenth grid does not
    b = Batch(pics)
    before = b.results()
    for stage in ("qp", "deblock", "sao"):
        recs, n = b.table(stage)
        assert getattr(b.L, ENTRIES[stage])(recs, n, None) == INVALID
        msg = b.L.kvz_hip_last_error().decode()
        assert ENTRIES[stage] in msg and "picture 13" in msg and "KVZ_HIP_CHAIN_TILE_BOUNDS" in msg, msg
    b.sync()
    for got, want in zip(b.results(), before):
        same(got, want, "after the overflow")
    # thirteen of them are a call, and the statistics take no grid: fourteen are one
    ok = Batch(pics[:13])
    ok.run(stages=("qp", "deblock", "sao"))
    b.call("stats")
    b.sync()
    ref = Pic(api, wide_state(12))
    Batch([ref]).singles()
    b.sync()
    same(pics[12].result(), ref.result(), "the thirteenth wide picture")


# ---------------------------------------------------------------- 6. the numpy conveniences
def test_numpy_conveniences_equal_the_ctypes_path(api):
    S = states()
    names = ["tile ragged", "qp coarse", "tile mono"]
    b = Batch([Pic(api, S[n], chain_rows=i & 1) for i, n in enumerate(names)])
    b.run()
    b.sync()
    want = b.results()
    tiles = lambda s: api.tile_grid(s["width"], s["height"], s["col_bd"], s["row_bd"]) if s["tiled"] else None
    maps = api.cu_qp_frames([dict(cus=S[n]["cus"], cbf=S[n]["cbf"], lcu_qp=S[n]["lcu_qp"], start_qp=S[n]["start_qp"], tiles=tiles(S[n]), chain_rows=i & 1)
                             for i, n in enumerate(names)])
    deb = api.deblock_frames([dict(y=S[n]["pred"][0], u=S[n]["pred"][1], v=S[n]["pred"][2], cus=m[0], prm=TC.chain_deblock_params(S[n]), tiles=tiles(S[n]))
                              for n, m in zip(names, maps)])
    stats = api.sao_stats_frames([dict(src=S[n]["src"], rec=d, chroma=S[n]["chroma"], with_cands=i != 1) for i, (n, d) in enumerate(zip(names, deb))])
    dst = api.sao_frames([dict(rec=d, sao_luma=S[n]["sao_luma"], sao_chroma=S[n]["sao_chroma"], chroma=S[n]["chroma"], tiles=tiles(S[n])) for n, d in zip(names, deb)])
    for i, w_ in enumerate(want):
        np.testing.assert_array_equal(maps[i][0].view(np.uint8).reshape(w_["cus"].shape), w_["cus"])
        np.testing.assert_array_equal(maps[i][1], w_["last"])
        TT.assert_planes(deb[i], w_["rec"], "deblock_frames %d" % i)
        TT.assert_planes(dst[i], w_["dst"], "sao_frames %d" % i)
        np.testing.assert_array_equal(stats[i][0].view(np.int32).reshape(-1), w_["stats"])
        assert (stats[i][1] is None) == (i == 1)
        if i != 1:
            np.testing.assert_array_equal(stats[i][1].view(np.int32).reshape(-1), w_["cands"])
    assert api.cu_qp_frames([]) == [] and api.sao_frames([]) == []
    s0 = S[names[0]]
    with pytest.raises(Exception, match="picture 1"):
        api.cu_qp_frames([dict(cus=s0["cus"], cbf=s0["cbf"], lcu_qp=s0["lcu_qp"], start_qp=30), dict(cus=s0["cus"], cbf=s0["cbf"], lcu_qp=s0["lcu_qp"], start_qp=99)])

"""GPU: kvz_hip_sao_stats_frame and kvz_hip_sao_frame against the committed fixture, on planes that are rectangles inside larger
buffers, against the existing block-list SAO entries on the device, on refused arguments, and in the chain kvz_hip_deblock_frame ->
kvz_hip_sao_stats_frame -> host pick -> kvz_hip_sao_frame on one stream, eager and replayed from a captured graph.  Every output
starts poisoned, every array is staged between guard bands, every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import sao_frame_cases as SC
from patterns import deblock_case, deblock_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sao_frame.npz")
GUARD, GUARD_BYTE = 512, 0xC3


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


class View:
    """a plane as the rectangle buf[top:top + h, left:left + w] of a 2-D uint8 buffer whose row length is the stride"""

    def __init__(self, buf, w=None, h=None, left=0, top=0):
        self.buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self.w, self.h = (self.buf.shape[1] if w is None else w), (self.buf.shape[0] if h is None else h)
        self.left, self.top = left, top

    stride = property(lambda self: self.buf.shape[1])
    offset = property(lambda self: self.top * self.stride + self.left)

    def crop(self, buf):
        return buf[self.top:self.top + self.h, self.left:self.left + self.w]


def embed(plane, stride, left, top, fill, bottom=3):
    h, w = plane.shape
    buf = np.full((top + h + bottom, stride), fill, np.uint8)
    buf[top:top + h, left:left + w] = plane
    return View(buf, w, h, left, top)


def poisoned(view_or_shape):
    if isinstance(view_or_shape, View):
        v = view_or_shape
        return View(np.full(v.buf.shape, SC.POISON_PIXEL, np.uint8), v.w, v.h, v.left, v.top)
    return View(np.full(view_or_shape, SC.POISON_PIXEL, np.uint8))


class Staged:
    """every array of the two calls in device memory between guard bands of GUARD bytes.  src, rec, dst: (y, u, v) planes as 2-D
    arrays or Views (dst default: compact, poisoned)"""

    def __init__(self, A, src, rec, luma, chro, chroma=1, dst=None):
        from kvazaar_amd import _lib
        self.A, self.L, self.check = A, _lib.init(0), _lib.check
        self.chroma, self.n = int(chroma), 3 if chroma else 1
        as_view = lambda p: p if isinstance(p, View) else View(p)
        self.src, self.rec = [as_view(p) for p in src[:self.n]], [as_view(p) for p in rec[:self.n]]
        self.w, self.h = self.rec[0].w, self.rec[0].h
        self.dst = [as_view(p) for p in dst[:self.n]] if dst is not None else [poisoned((v.h, v.w)) for v in self.rec]
        self.n_lcu = A.lcu_count(self.w, self.h)
        words = lambda n: np.full(n, SC.POISON_WORD, np.uint32).view(np.int32)
        self.host = {"src": [v.buf for v in self.src], "rec": [v.buf for v in self.rec], "dst": [v.buf for v in self.dst],
                     "luma": [np.ascontiguousarray(luma, dtype=np.int32).reshape(self.n_lcu, 14)],
                     "chro": [np.ascontiguousarray(chro, dtype=np.int32).reshape(self.n_lcu, 14)] if chroma else [],
                     "stats": [words(self.n * self.n_lcu * 104)], "cands": [words(self.n * self.n_lcu * 30)]}
        self.dev = {k: [self._up(a) for a in v] for k, v in self.host.items()}
        self.table = A.ref_picture_table([(self.ptr("src", 0), self.ptr("src", 1), self.ptr("src", 2), self.src[0].stride,
                                           self.src[1].stride if chroma else 0)], self.w, self.h)

    def _up(self, a):
        raw = np.full(a.nbytes + 2 * GUARD, GUARD_BYTE, np.uint8)
        raw[GUARD:GUARD + a.nbytes] = a.view(np.uint8).reshape(-1)
        return self.A.DeviceBuffer.from_numpy(raw)

    def ptr(self, kind, k=0):
        if k >= len(self.dev[kind]):
            return None
        views = getattr(self, kind, None)
        return self.dev[kind][k].ptr + GUARD + (views[k].offset if isinstance(views, list) else 0)

    def upload(self, kind, k, a, stream=None):
        a = np.ascontiguousarray(a)
        assert a.nbytes == self.host[kind][k].nbytes
        self.check(self.L.kvz_hip_memcpy_h2d(self.dev[kind][k].ptr + GUARD, a.ctypes.data, a.nbytes, stream), "h2d")
        self._keep = getattr(self, "_keep", []) + [a]
        self.host[kind][k] = a.view(self.host[kind][k].dtype).reshape(self.host[kind][k].shape)

    def stats_call(self, stream=None, **over):
        a = {"table": self.table.ctypes.data, "y": self.ptr("rec", 0), "sy": self.rec[0].stride, "u": self.ptr("rec", 1), "v": self.ptr("rec", 2),
             "sc": self.rec[1].stride if self.chroma else 0, "chroma": self.chroma, "stats": self.ptr("stats"), "cands": self.ptr("cands")}
        a.update(over)
        return self.L.kvz_hip_sao_stats_frame(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["chroma"], a["stats"], a["cands"], stream)

    def frame_call(self, stream=None, **over):
        a = {"y": self.ptr("rec", 0), "sy": self.rec[0].stride, "u": self.ptr("rec", 1), "v": self.ptr("rec", 2),
             "sc": self.rec[1].stride if self.chroma else 0, "dy": self.ptr("dst", 0), "dsy": self.dst[0].stride, "du": self.ptr("dst", 1),
             "dv": self.ptr("dst", 2), "dsc": self.dst[1].stride if self.chroma else 0, "w": self.w, "h": self.h, "luma": self.ptr("luma"),
             "chro": self.ptr("chro"), "chroma": self.chroma}
        a.update(over)
        return self.L.kvz_hip_sao_frame(a["y"], a["sy"], a["u"], a["v"], a["sc"], a["dy"], a["dsy"], a["du"], a["dv"], a["dsc"], a["w"], a["h"],
                                        a["luma"], a["chro"], a["chroma"], stream)

    def download(self, kind, k):
        a = self.host[kind][k]
        raw = self.dev[kind][k].to_numpy(np.uint8, (a.nbytes + 2 * GUARD,))
        assert (raw[:GUARD] == GUARD_BYTE).all() and (raw[GUARD + a.nbytes:] == GUARD_BYTE).all(), "guard band of %s %d" % (kind, k)
        return raw[GUARD:GUARD + a.nbytes].view(a.dtype).reshape(a.shape)

    def result(self):
        """-> {"stats", "cands", "dst", "dst_buf"}; asserts every guard band, that no input changed and that nothing of a destination
        buffer outside its plane (stride padding included) changed"""
        for kind in ("src", "rec", "luma", "chro"):
            for k, a in enumerate(self.host[kind]):
                np.testing.assert_array_equal(self.download(kind, k), a, err_msg="%s %d was written" % (kind, k))
        bufs = [self.download("dst", k) for k in range(self.n)]
        for k, (v, b) in enumerate(zip(self.dst, bufs)):
            outside = np.ones(b.shape, bool)
            outside[v.top:v.top + v.h, v.left:v.left + v.w] = False
            np.testing.assert_array_equal(b[outside], self.host["dst"][k][outside], err_msg="dst %d outside the plane" % k)
        pad = [None] * (3 - self.n)
        return {"stats": self.download("stats", 0).view(SC.STATS).reshape(self.n, self.n_lcu),
                "cands": self.download("cands", 0).view(SC.CAND).reshape(self.n, self.n_lcu),
                "dst": tuple([v.crop(b) for v, b in zip(self.dst, bufs)] + pad), "dst_buf": bufs}

    def run(self):
        self.check(self.stats_call(), "sao_stats_frame")
        self.check(self.frame_call(), "sao_frame")
        self.check(self.L.kvz_hip_stream_sync(None), "sync")
        return self.result()


def assert_equal(got, want, what, chroma=1):
    np.testing.assert_array_equal(got["stats"].view(np.int32), want["stats"].view(np.int32), err_msg=what + " stats")
    np.testing.assert_array_equal(got["cands"].view(np.int32), want["cands"].view(np.int32), err_msg=what + " cands")
    for k in range(3 if chroma else 1):
        np.testing.assert_array_equal(got["dst"][k], want["dst"][k], err_msg="%s dst %d" % (what, k))


@pytest.mark.parametrize("pic", SC.FIXTURE_PICTURES, ids=[p[0] for p in SC.FIXTURE_PICTURES])
def test_every_output_equals_the_committed_fixture(api, golden, pic):
    name, w, h, chroma, seed = pic
    src, rec, luma, chro, want = SC.load_fixture_case(golden, name, chroma)
    st = Staged(api, src, rec, luma, chro, chroma)
    assert_equal(st.run(), want, name, chroma)
    assert len(st.dev["dst"]) == (3 if chroma else 1)           # 4:0:0: there is no U / V to write
    # the numpy conveniences
    stats, cands = api.sao_stats_frame(src, rec, chroma)
    dst = api.sao_frame(rec, luma, chro, chroma)
    assert_equal({"stats": stats, "cands": cands, "dst": dst}, want, name + " convenience", chroma)
    assert api.sao_stats_frame(src, rec, chroma, with_cands=False)[1] is None


def test_4_0_0_ignores_the_chroma_arguments(api, golden):
    """chroma == 0 with chroma pointers handed in all the same: U / V destinations stay poisoned, one record per LCU is written"""
    src, rec, luma, chro, want = SC.load_fixture_case(golden, "one", 1)
    st = Staged(api, src, rec, luma, chro, 1)
    st.check(st.stats_call(chroma=0), "sao_stats_frame")
    st.check(st.frame_call(chroma=0), "sao_frame")
    st.check(st.L.kvz_hip_stream_sync(None), "sync")
    got = st.result()
    np.testing.assert_array_equal(got["dst"][0], want["dst"][0])
    assert (got["dst"][1] == SC.POISON_PIXEL).all() and (got["dst"][2] == SC.POISON_PIXEL).all()
    np.testing.assert_array_equal(got["stats"][0].view(np.int32), want["stats"][0].view(np.int32))
    assert (got["stats"][1:].view(np.uint32) == SC.POISON_WORD).all() and (got["cands"][1:].view(np.uint32) == SC.POISON_WORD).all()


def test_planes_inside_larger_buffers_with_strides_of_their_own(api, golden):
    """the ragged picture as a rectangle at a 4-byte aligned, non-zero offset inside larger buffers: four different strides for source
    Y / C and rec Y / C, destination strides different from rec's.  The bytes right of the width of rec are poisoned differently in two
    runs and the outputs agree: they are not read.  result() checks that nothing outside the rectangles is written."""
    src, rec, luma, chro, want = SC.load_fixture_case(golden, "ragged", 1)
    outs = []
    for fill in (0x11, 0xEE):
        vs = [embed(src[0], 236, 12, 2, fill ^ 0xFF)] + [embed(p, 124, 8, 1, fill ^ 0xFF) for p in src[1:]]
        vr = [embed(rec[0], 260, 20, 3, fill)] + [embed(p, 144, 4, 2, fill) for p in rec[1:]]
        vd = [poisoned(embed(rec[0], 224, 16, 1, 0))] + [poisoned(embed(p, 112, 12, 2, 0)) for p in rec[1:]]
        assert len({vs[0].stride, vs[1].stride, vr[0].stride, vr[1].stride}) == 4 and vd[0].stride != vr[0].stride and vd[1].stride != vr[1].stride
        assert all(v.offset % 4 == 0 and v.offset > 0 and v.stride % 4 == 0 for v in vs + vr + vd)
        got = Staged(api, vs, vr, luma, chro, 1, dst=vd).run()
        assert_equal(got, want, "embedded, fill %#x" % fill)
        outs.append(got)
    for k in range(3):
        np.testing.assert_array_equal(outs[0]["dst_buf"][k], outs[1]["dst_buf"][k])


@pytest.mark.parametrize("name", ["ragged", "tiny"])
def test_equals_the_block_list_entries_on_the_device(api, golden, name):
    """no reference involved: the statistics against kvz_hip_sao_edge_stats_batch / _band_stats_batch on host-blitted blocks, the
    reconstruction against one kvz_hip_sao_reconstruct_color_batch per plane with host-trimmed rectangles on top of a copy"""
    w, h = {p[0]: (p[1], p[2]) for p in SC.FIXTURE_PICTURES}[name]
    src, rec, luma, chro, _ = SC.load_fixture_case(golden, name, 1)
    got = Staged(api, src, rec, luma, chro, 1).run()
    for color in range(3):
        blocks = SC.lcu_blocks(w, h, color)
        for shape in sorted({b[2:] for b in blocks}):
            idx = [i for i, b in enumerate(blocks) if b[2:] == shape]
            o = np.stack([SC.blit(src[color], *blocks[i]).reshape(-1) for i in idx])
            r = np.stack([SC.blit(rec[color], *blocks[i]).reshape(-1) for i in idx])
            np.testing.assert_array_equal(got["stats"][color, idx]["edge"], api.sao_edge_stats_batch(o, r, shape[0], shape[1]))
            np.testing.assert_array_equal(got["stats"][color, idx]["band"], api.sao_band_stats_batch(o, r, shape[0], shape[1]))
        infos = luma if color == 0 else chro
        ph, pw = rec[color].shape
        rects = []
        for i, (x, y, bw, bh) in enumerate(blocks):
            eff = SC.effective(infos[i], color)
            if eff is None:
                continue
            if eff[0] == 2:
                x, y, bw, bh = SC.trim(x, y, bw, bh, eff[1], pw, ph)
            if bw > 0 and bh > 0:
                rects.append((x, y, bw, bh, i))
        assert rects
        np.testing.assert_array_equal(got["dst"][color], api.sao_reconstruct_color_batch(rec[color], rects, infos, color), err_msg="plane %d" % color)


def test_refused_arguments_write_nothing(api, golden):
    src, rec, luma, chro, want = SC.load_fixture_case(golden, "ragged", 1)
    # strides with room for the stride cases below
    vs = [embed(src[0], 208, 0, 0, 1, 0)] + [embed(p, 104, 0, 0, 1, 0) for p in src[1:]]
    vr = [embed(rec[0], 208, 0, 0, 2, 0)] + [embed(p, 104, 0, 0, 2, 0) for p in rec[1:]]
    vd = [poisoned(v) for v in vr]
    st = Staged(api, vs, vr, luma, chro, 1, dst=vd)
    A, w, h = api, 200, 136
    tbl = lambda planes, ww=w, hh=h: A.ref_picture_table([planes], ww, hh)
    sp = (st.ptr("src", 0), st.ptr("src", 1), st.ptr("src", 2), 208, 104)
    tables = [tbl(sp, w - 4), tbl(sp, w, h - 4), tbl(sp, 4, 8), tbl((sp[0] + 2,) + sp[1:]), tbl(sp[:3] + (206, 104)), tbl(sp[:3] + (196, 104)),
              tbl((0,) + sp[1:]), tbl(sp[:2] + (0,) + sp[3:]), tbl(sp[:3] + (208, 96)), tbl((sp[0], sp[1] + 1) + sp[2:])]
    rcs = [("stats", st.stats_call(table=t.ctypes.data)) for t in tables]
    rcs += [("stats", rc) for rc in (
        st.stats_call(table=None), st.stats_call(y=None), st.stats_call(u=None), st.stats_call(v=None), st.stats_call(stats=None),
        st.stats_call(y=st.ptr("rec", 0) + 1), st.stats_call(y=st.ptr("rec", 0) + 2), st.stats_call(v=st.ptr("rec", 2) + 2),      # misaligned plane
        st.stats_call(sy=206), st.stats_call(sc=102),                                                                             # misaligned stride
        st.stats_call(sy=196), st.stats_call(sc=96))]                                                                             # stride below width
    rcs += [("frame", rc) for rc in (
        st.frame_call(y=None), st.frame_call(u=None), st.frame_call(v=None), st.frame_call(dy=None), st.frame_call(du=None), st.frame_call(dv=None),
        st.frame_call(luma=None), st.frame_call(chro=None),
        st.frame_call(y=st.ptr("rec", 0) + 2), st.frame_call(dy=st.ptr("dst", 0) + 1), st.frame_call(du=st.ptr("dst", 1) + 2),    # misaligned plane
        st.frame_call(sy=206), st.frame_call(dsy=206), st.frame_call(sc=102), st.frame_call(dsc=102),                             # misaligned stride
        st.frame_call(w=196), st.frame_call(h=132), st.frame_call(w=4), st.frame_call(h=0),                                       # not a multiple of 8 / below 8
        st.frame_call(sy=196), st.frame_call(dsy=192), st.frame_call(sc=96), st.frame_call(dsc=96),                               # stride below width
        st.frame_call(dy=st.ptr("rec", 0)), st.frame_call(du=st.ptr("rec", 1)), st.frame_call(dv=st.ptr("rec", 2)))]               # in place
    for i, (which, rc) in enumerate(rcs):
        assert rc == -2, "refusal %d (%s) returned %d" % (i, which, rc)
    assert b"kvz_hip_sao_frame" in st.L.kvz_hip_last_error()
    st.check(st.L.kvz_hip_stream_sync(None), "sync")
    got = st.result()
    assert (got["stats"].view(np.uint32) == SC.POISON_WORD).all() and (got["cands"].view(np.uint32) == SC.POISON_WORD).all()
    assert all((b == SC.POISON_PIXEL).all() for b in got["dst_buf"])
    assert st.L.kvz_hip_abi_version() == 4
    # cands is optional
    st.check(st.stats_call(cands=None), "sao_stats_frame without cands")
    st.check(st.L.kvz_hip_stream_sync(None), "sync")
    got = st.result()
    np.testing.assert_array_equal(got["stats"].view(np.int32), want["stats"].view(np.int32))
    assert (got["cands"].view(np.uint32) == SC.POISON_WORD).all()


def chain_picture(seed, w=256, h=192, qp=34):
    """patterns' deblock case with a source -> (src, undeblocked planes, cus, params, deblocked planes).  The source is the picture
    smoothed (3 x 3 mean) in two of three LCUs, where edge offsets pay, and the picture + noise in the others, where they do not"""
    y, u, v, cus = deblock_case(w, h, seed, qp=qp)
    g = np.random.default_rng(seed + 1)

    def source(p, lcu):
        q = np.pad(p.astype(int), 1, mode="edge")
        mean = sum(q[1 + dy:1 + dy + p.shape[0], 1 + dx:1 + dx + p.shape[1]] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) // 9
        yy, xx = np.mgrid[0:p.shape[0], 0:p.shape[1]]
        noisy = (yy // lcu + xx // lcu) % 3 == 0
        return np.clip(np.where(noisy, p + g.integers(-6, 7, p.shape), mean + g.integers(-2, 3, p.shape)), 0, 255).astype(np.uint8)
    src = (source(y, 64), source(u, 32), source(v, 32))
    prm = deblock_params(qp=qp, chroma=1)
    return src, (y, u, v), cus, prm, O.deblock_frame(y, u, v, cus, prm)


def test_deblock_stats_pick_reconstruct_on_one_stream_and_replayed_from_a_graph(api):
    w, h = 256, 192
    src, planes, cus, prm, deb = chain_picture(910)
    want_stats = SC.compose_stats(src, deb, 1)
    want_cands = SC.compose_cands(want_stats)
    luma, chro = SC.pick_edge_records(want_cands, 1)
    assert {0, 2} <= set(luma[:, 0]) | set(chro[:, 0]) and len(set(luma[luma[:, 0] == 2, 1])) > 1
    want = {"stats": want_stats, "cands": want_cands, "dst": SC.compose_recon(deb, luma, chro, 1)}
    zeros = np.zeros((SC.lcu_grid(w, h)[0] * SC.lcu_grid(w, h)[1], 14), np.int32)
    st = Staged(api, src, planes, zeros, zeros, 1)
    L = st.L
    dcus = api.DeviceBuffer.from_numpy(np.ascontiguousarray(cus).view(np.uint8))
    s, graph = L.kvz_hip_stream_create(), C.c_void_p()
    try:
        st.check(L.kvz_hip_deblock_frame(st.ptr("rec", 0), w, st.ptr("rec", 1), st.ptr("rec", 2), w // 2, w, h, dcus.ptr, prm.ctypes.data, s), "deblock_frame")
        st.check(st.stats_call(s), "sao_stats_frame")
        n = st.host["cands"][0].nbytes
        got_c = np.empty(n // 4, np.int32)
        st.check(L.kvz_hip_memcpy_d2h(got_c.ctypes.data, st.ptr("cands"), n, s), "d2h")
        st.check(L.kvz_hip_stream_sync(s), "sync")
        pick = SC.pick_edge_records(got_c.view(SC.CAND).reshape(3, -1), 1)               # the host's part of the chain
        st.upload("luma", 0, pick[0], s)
        st.upload("chro", 0, pick[1], s)
        st.check(st.frame_call(s), "sao_frame")
        st.check(L.kvz_hip_stream_sync(s), "sync")
        st.host["rec"] = [np.ascontiguousarray(p) for p in deb]                          # the planes were deblocked in place
        assert_equal(st.result(), want, "chain")
        np.testing.assert_array_equal(pick[0], luma)
        np.testing.assert_array_equal(pick[1], chro)

        # both SAO calls captured once as a linear chain, replayed after the planes and the records were overwritten
        st.check(L.kvz_hip_graph_begin(s), "graph_begin")
        st.check(st.stats_call(s), "sao_stats_frame")
        st.check(st.frame_call(s), "sao_frame")
        st.check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        for seed in (900, 920):
            src2, _, _, _, deb2 = chain_picture(seed)
            luma2, chro2 = SC.make_records(w, h, seed + 2, 0), SC.make_records(w, h, seed + 3, 1)
            for k in range(3):
                st.upload("src", k, src2[k], s)
                st.upload("rec", k, deb2[k], s)
                st.upload("dst", k, np.full_like(st.host["dst"][k], SC.POISON_PIXEL), s)
            st.upload("luma", 0, luma2, s)
            st.upload("chro", 0, chro2, s)
            st.upload("stats", 0, np.full_like(st.host["stats"][0].view(np.uint32), SC.POISON_WORD), s)
            st.upload("cands", 0, np.full_like(st.host["cands"][0].view(np.uint32), SC.POISON_WORD), s)
            st.check(L.kvz_hip_stream_sync(s), "sync")
            st.check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            st.check(L.kvz_hip_stream_sync(s), "sync")
            stats2 = SC.compose_stats(src2, deb2, 1)
            assert_equal(st.result(), {"stats": stats2, "cands": SC.compose_cands(stats2), "dst": SC.compose_recon(deb2, luma2, chro2, 1)},
                         "replay of picture %d" % seed)
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)

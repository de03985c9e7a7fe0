"""GPU: kvz_hip_inter_residual_frame against the committed fixture, against the composition of the reference's own functions at frame
scale (tests/inter_residual_cases.py), against the existing contiguous entry over the same TU population, and in the chain
kvz_hip_inter_recon_frame -> kvz_hip_inter_residual_frame -> kvz_hip_deblock_frame on one stream, eager and replayed from a
captured graph.  Every output starts poisoned, every array is staged between guard bands, every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import inter_recon_cases as IC
import inter_residual_cases as RC
import oracle_lib as O
from patterns import CU_INFO, deblock_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_residual.npz")
GUARD, GUARD_BYTE = 512, 0xC3


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


class Staged:
    """every array of one call in device memory between guard bands of GUARD bytes"""

    def __init__(self, A, src, pred, cus, qp, chroma=1, signhide=0, slice_is_intra=0, init=None, scaling_list=0):
        from kvazaar_amd import _lib
        self.A, self.L = A, _lib.init(0)
        self.chroma, self.n = int(chroma), 3 if chroma else 1
        self.h, self.w = src[0].shape
        init = init or RC.initial_outputs(self.w, self.h, chroma)
        self.host = {"src": [np.ascontiguousarray(p) for p in src[:self.n]], "rec": [np.ascontiguousarray(p) for p in pred[:self.n]],
                     "coeff": [np.ascontiguousarray(c) for c in init[0][:self.n]], "cus": [np.ascontiguousarray(cus)],
                     "cbf_out": [np.ascontiguousarray(init[1])], "costs": [np.ascontiguousarray(init[2])]}
        self.dev = {k: [self._up(a) for a in v] for k, v in self.host.items()}
        self.prm = A.inter_residual_params(qp, slice_is_intra, signhide, chroma, scaling_list)
        self.table = A.ref_picture_table([(self.ptr("src", 0), self.ptr("src", 1), self.ptr("src", 2), self.host["src"][0].shape[1],
                                           self.host["src"][1].shape[1] if chroma else 0)], self.w, self.h)

    def _up(self, a):
        raw = np.full(a.nbytes + 2 * GUARD, GUARD_BYTE, np.uint8)
        raw[GUARD:GUARD + a.nbytes] = a.view(np.uint8).reshape(-1)
        return self.A.DeviceBuffer.from_numpy(raw)

    def ptr(self, kind, k=0):
        return self.dev[kind][k].ptr + GUARD if k < len(self.dev[kind]) else None

    def upload(self, kind, k, a, stream=None):
        a = np.ascontiguousarray(a)
        assert a.nbytes == self.host[kind][k].nbytes
        from kvazaar_amd import _lib
        _lib.check(self.L.kvz_hip_memcpy_h2d(self.ptr(kind, k), a.ctypes.data, a.nbytes, stream), "h2d")
        self._keep = getattr(self, "_keep", []) + [a]

    def call(self, stream=None, **over):
        a = {"table": self.table.ctypes.data, "y": self.ptr("rec", 0), "sy": self.host["rec"][0].shape[1], "u": self.ptr("rec", 1), "v": self.ptr("rec", 2),
             "sc": self.host["rec"][1].shape[1] if self.chroma else 0, "cus": self.ptr("cus"), "cy": self.ptr("coeff", 0), "cu": self.ptr("coeff", 1),
             "cv": self.ptr("coeff", 2), "cbf": self.ptr("cbf_out"), "costs": self.ptr("costs"), "prm": self.prm.ctypes.data}
        a.update(over)
        return self.L.kvz_hip_inter_residual_frame(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["cy"], a["cu"], a["cv"], a["cbf"],
                                                   a["costs"], a["prm"], stream)

    def raw(self, kind, k):
        a = self.host[kind][k]
        return self.dev[kind][k].to_numpy(np.uint8, (a.nbytes + 2 * GUARD,))

    def result(self):
        """-> outputs as RC.compose returns them; asserts every guard band (inputs included)"""
        out = {}
        for kind, bufs in self.dev.items():
            got = []
            for k, a in enumerate(self.host[kind]):
                raw = self.raw(kind, k)
                assert (raw[:GUARD] == GUARD_BYTE).all() and (raw[GUARD + a.nbytes:] == GUARD_BYTE).all(), "guard band of %s %d" % (kind, k)
                got.append(raw[GUARD:GUARD + a.nbytes].view(a.dtype).reshape(a.shape))
            out[kind] = got
        pad = [None] * (3 - self.n)
        for kind in ("src",):
            for g, a in zip(out[kind], self.host[kind]):
                np.testing.assert_array_equal(g, a, err_msg="the source was written")
        return {"rec": tuple(out["rec"] + pad), "coeff": tuple(out["coeff"] + pad), "cus": out["cus"][0], "cbf_out": out["cbf_out"][0],
                "costs": out["costs"][0]}


def run(A, src, pred, cus, qp, chroma=1, signhide=0, **kw):
    st = Staged(A, src, pred, cus, qp, chroma, signhide, **kw)
    from kvazaar_amd import _lib
    _lib.check(st.call(), "inter_residual_frame")
    _lib.check(st.L.kvz_hip_stream_sync(None), "sync")
    return st.result()


def test_every_output_equals_the_committed_fixture(api):
    z = np.load(GOLDEN, allow_pickle=False)
    for (name, w, h, chroma, qp, signhide, seed) in RC.FIXTURE_PICTURES:
        src, pred, cus, want = RC.load_fixture_case(z, name, chroma)
        RC.assert_outputs_equal(run(api, src, pred, cus, qp, chroma, signhide), want, name, chroma)
        # the numpy convenience, over zeroed outputs: the same inside the inter CUs
        conv = api.inter_residual_frame(src, pred, cus, qp, chroma, signhide=signhide)
        zero = RC.compose(src, pred, cus, qp, chroma, signhide)
        RC.assert_outputs_equal(conv, zero, name + " convenience", chroma)


def frame_case(w, h, seed, chroma, pad=0):
    cus, _ = RC.make_map(w, h, seed, intra_share=0.08, blank_share=0.05)
    pred = RC.smooth_planes(w, h, seed + 1, chroma, pad=pad)
    return RC.make_source(pred, cus, seed + 2, chroma), pred, cus


@pytest.mark.parametrize("chroma", [1, 0])
@pytest.mark.parametrize("signhide", [0, 1])
@pytest.mark.parametrize("qp", [22, 37])
def test_full_hd_frame_equals_the_composed_oracle(api, qp, signhide, chroma):
    """1920x1080: the last LCU row is ragged (1080 = 16 * 64 + 56); every output, every element"""
    w, h = 1920, 1080
    src, pred, cus = frame_case(w, h, 300 + qp + signhide, chroma)
    init = RC.initial_outputs(w, h, chroma)
    want = RC.compose(src, pred, cus, qp, chroma, signhide, init=init, many=True)
    assert len({t[:2] for t in want["tus"]}) == (10 if chroma else 4) and {t[2] for t in want["tus"]} == {0, 1}
    RC.assert_outputs_equal(run(api, src, pred, cus, qp, chroma, signhide, init=init), want, "1080p", chroma)


def test_4k_frame_equals_the_composed_oracle(api):
    w, h = 3840, 2160
    src, pred, cus = frame_case(w, h, 400, 1)
    init = RC.initial_outputs(w, h, 1)
    want = RC.compose(src, pred, cus, 32, 1, 1, init=init, many=True)
    RC.assert_outputs_equal(run(api, src, pred, cus, 32, 1, 1, init=init), want, "4k")


@pytest.mark.parametrize("signhide", [0, 1])
def test_equals_the_contiguous_cost_entry_over_the_same_tus(api, signhide):
    """the same TU population gathered on the host, through kvz_hip_quantize_residual_cost_batch per size and plane"""
    w, h, qp = 448, 264, 27
    src, pred, cus = frame_case(w, h, 500, 1)
    init = RC.initial_outputs(w, h, 1)

    def through_batch(ref_b, pred_b, n, p):
        return api.quantize_residual_batch(ref_b, pred_b, n, qp, p, 0, 0, 0, signhide, with_costs=True)
    want = RC.compose(src, pred, cus, qp, 1, signhide, init=init, quantize=through_batch)
    RC.assert_outputs_equal(run(api, src, pred, cus, qp, 1, signhide, init=init), want, "frame vs cost batch")


def inter_masks(cus, w, h):
    m = np.zeros((h, w), bool)
    for (x, y, s) in RC.inter_cus(cus, w, h):
        m[y:y + s, x:x + s] = True
    return m, m[::2, ::2], m[::4, ::4]


@pytest.mark.parametrize("chroma", [1, 0])
def test_everything_outside_the_inter_cus_is_untouched(api, chroma):
    w, h, pad = 200, 136, 12
    src, pred, cus = frame_case(w, h, 600, chroma, pad=pad)
    got = run(api, src, pred, cus, 30, chroma, 0)
    m, mc, ms = inter_masks(cus, w, h)
    assert m.any() and not m.all()
    assert ((cus["type"] == IC.CU_INTER) & ~ms).any() and (cus["type"] == IC.CU_INTRA).any() and (cus["type"] == 0).any()
    for k in range(3 if chroma else 1):
        mk, pw = (mc, w // 2) if k else (m, w)
        assert (got["rec"][k][:, pw:] == RC.POISON_PIXEL).all(), "wrote between width and stride"
        np.testing.assert_array_equal(got["rec"][k][:, :pw][~mk], pred[k][:, :pw][~mk])
        assert not np.array_equal(got["rec"][k][:, :pw][mk], pred[k][:, :pw][mk])
        # coefficients: the LCU arrays in picture order (z-order undone per 4x4 block)
        lw = 32 if k else 64
        cov = np.zeros((((h + 63) // 64) * lw, ((w + 63) // 64) * lw), bool)
        cov[:mk.shape[0], :mk.shape[1]] = mk
        c = got["coeff"][k]
        lx = (w + 63) // 64
        for lcu in range(c.shape[0]):
            for by in range(0, lw, 4):
                for bx in range(0, lw, 4):
                    z = RC.xy_to_zorder(lw, bx, by)
                    inside = cov[(lcu // lx) * lw + by, (lcu % lx) * lw + bx]
                    assert inside or (c[lcu, z:z + 16] == RC.POISON_COEFF).all(), "coefficients of LCU %d block (%d, %d)" % (lcu, bx, by)
    assert (got["cbf_out"][~ms] == RC.POISON_CBF).all() and (got["cbf_out"][ms] <= (7 if chroma else 1)).all()
    tl = np.zeros(ms.shape, bool)
    for (x, y, s) in RC.inter_cus(cus, w, h):
        tl[y // 4, x // 4] = True
    assert (got["costs"].view(np.uint32).reshape(ms.shape + (6,))[~tl] == RC.POISON_COST).all()
    assert (got["costs"].view(np.uint32).reshape(ms.shape + (6,))[tl] != RC.POISON_COST).all()
    # the records: nothing but cbf_y of the inter CUs changed
    before, after = np.array(cus), np.array(got["cus"])
    np.testing.assert_array_equal(after[~ms].view(np.uint8), before[~ms].view(np.uint8))
    before["cbf_y"], after["cbf_y"] = 0, 0
    np.testing.assert_array_equal(after.view(np.uint8), before.view(np.uint8))
    RC.assert_outputs_equal(got, RC.compose(src, pred, cus, 30, chroma, 0, init=RC.initial_outputs(w, h, chroma)), "padded", chroma)


def test_inconsistent_map_stays_inside_the_arrays(api):
    """records that disagree inside a CU (random depth / tr_depth / type per SCU): the output there is unspecified, the guard bands
    (checked by result()) and the area between width and stride are intact"""
    w, h = 200, 136
    g = np.random.default_rng(7)
    cus = np.zeros((h // 4, w // 4), dtype=CU_INFO)
    cus["type"] = g.integers(0, 3, cus.shape)
    cus["depth"] = g.integers(0, 6, cus.shape)
    cus["tr_depth"] = g.integers(0, 256, cus.shape)
    cus["part_size"] = g.integers(0, 9, cus.shape)
    pred = RC.smooth_planes(w, h, 8, 1, pad=20)
    src = RC.smooth_planes(w, h, 9, 1)
    got = run(api, src, pred, cus, 26, 1, 1)
    for k in range(3):
        assert (got["rec"][k][:, (w >> (1 if k else 0)):] == RC.POISON_PIXEL).all()


def chain_case(w, h, seed, slice_b, n_refs):
    refs = IC.random_planes(w, h, seed, n_refs)
    cus, ref_LX = RC.make_map(w, h, seed + 1, n_refs=n_refs, slice_b=slice_b, intra_share=0.1, blank_share=0.0, bad_share=0.0, edge_cu=False)
    dest = tuple(np.full((h >> (1 if k else 0), w >> (1 if k else 0)), RC.POISON_PIXEL, np.uint8) for k in range(3))
    pred = IC.compose(refs, IC.walk_pus(cus, ref_LX, w, h), (h, w), 1, dest)
    src = RC.make_source(pred, cus, seed + 2, 1)
    return refs, cus, ref_LX, dest, pred, src


def chain_expected(pred, src, cus, ref_LX, qp, slice_b):
    mid = RC.compose(src, pred, cus, qp, 1, 0, many=True)
    prm = deblock_params(qp=qp, slice_is_b=int(slice_b), chroma=1)
    prm["ref_LX"] = ref_LX
    return mid, prm, O.deblock_frame(mid["rec"][0], mid["rec"][1], mid["rec"][2], mid["cus"], prm)


class Chain:
    """the three calls on device arrays that stay put: reference pictures, source, rec planes, CU array, coefficients"""

    def __init__(self, A, refs, cus, ref_LX, dest, src, qp, slice_b):
        from kvazaar_amd import _lib
        self.A, self.L, self.check = A, _lib.init(0), _lib.check
        self.h, self.w = src[0].shape
        self.recon = A._Recon(refs, (self.h, self.w), 1, dest)
        self.st = Staged(A, src, dest, cus, qp, 1, 0, init=(tuple(np.zeros_like(c) for c in RC.initial_outputs(self.w, self.h)[0]),
                                                             np.zeros(cus.shape, np.uint8), np.zeros(cus.shape, RC.COST)))
        self.rprm = np.zeros(1, dtype=A.INTER_RECON_PARAMS)
        self.rprm["chroma"], self.rprm["n_refs"], self.rprm["ref_LX"] = 1, len(refs), ref_LX
        self.dprm = deblock_params(qp=qp, slice_is_b=int(slice_b), chroma=1)
        self.dprm["ref_LX"] = ref_LX

    def launch(self, s):
        st, w, h = self.st, self.w, self.h
        self.check(self.L.kvz_hip_inter_recon_frame(st.ptr("rec", 0), w, st.ptr("rec", 1), st.ptr("rec", 2), w // 2, w, h, st.ptr("cus"),
                                                    self.recon.table.ctypes.data, self.rprm.ctypes.data, s), "inter_recon_frame")
        self.check(st.call(s), "inter_residual_frame")
        self.check(self.L.kvz_hip_deblock_frame(st.ptr("rec", 0), w, st.ptr("rec", 1), st.ptr("rec", 2), w // 2, w, h, st.ptr("cus"),
                                                self.dprm.ctypes.data, s), "deblock_frame")


@pytest.mark.parametrize("slice_b", [False, True], ids=["P", "B"])
def test_prediction_residual_deblocking_on_one_stream(api, slice_b):
    w, h, qp, n_refs = 192, 128, 30, 2
    refs, cus, ref_LX, dest, pred, src = chain_case(w, h, 700 + slice_b, slice_b, n_refs)
    mid, prm, want = chain_expected(pred, src, cus, ref_LX, qp, slice_b)
    ch = Chain(api, refs, cus, ref_LX, dest, src, qp, slice_b)
    s = ch.L.kvz_hip_stream_create()
    try:
        ch.launch(s)                                       # three asynchronous calls, nothing between them
        ch.check(ch.L.kvz_hip_stream_sync(s), "sync")
        got = ch.st.result()
    finally:
        ch.L.kvz_hip_stream_destroy(s)
    for k in range(3):
        np.testing.assert_array_equal(got["rec"][k], want[k], err_msg="plane %d after the chain" % k)
        np.testing.assert_array_equal(got["coeff"][k], mid["coeff"][k])
    np.testing.assert_array_equal(got["cus"].view(np.uint8), mid["cus"].view(np.uint8))
    np.testing.assert_array_equal(got["costs"].view(np.uint32), mid["costs"].view(np.uint32))


def test_captured_chain_replays_on_another_picture(api):
    """the three calls captured once, replayed after the CU array, the source and the reference pictures were overwritten"""
    w, h, qp, n_refs = 192, 128, 30, 2
    first = chain_case(w, h, 800, True, n_refs)
    second = chain_case(w, h, 810, True, n_refs)
    ref_LX = first[2]
    refs2, cus2, _, dest, _, _ = second
    # the second picture under the first one's ref_LX (params are copied at capture): its prediction and source follow from that
    pred2 = IC.compose(refs2, IC.walk_pus(cus2, ref_LX, w, h), (h, w), 1, dest)
    src2 = RC.make_source(pred2, cus2, 812, 1)
    ch = Chain(api, first[0], first[1], ref_LX, dest, first[5], qp, True)
    L, s, graph = ch.L, ch.L.kvz_hip_stream_create(), C.c_void_p()
    ch.check(L.kvz_hip_graph_begin(s), "graph_begin")
    ch.launch(s)
    ch.check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
    assert graph.value
    try:
        for (refs, cus, src, pred) in ((first[0], first[1], first[5], first[4]), (refs2, cus2, src2, pred2)):
            for i, r in enumerate(refs):
                for k in range(3):
                    a = np.ascontiguousarray(r[k])
                    ch.check(L.kvz_hip_memcpy_h2d(ch.recon.keep[3 * i + k].ptr, a.ctypes.data, a.nbytes, s), "h2d")
            for k in range(3):
                ch.st.upload("src", k, src[k], s)
                ch.st.upload("rec", k, dest[k], s)
                ch.st.upload("coeff", k, np.zeros_like(ch.st.host["coeff"][k]), s)
            ch.st.upload("cus", 0, cus, s)
            ch.check(L.kvz_hip_stream_sync(s), "sync")
            ch.check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            ch.check(L.kvz_hip_stream_sync(s), "sync")
            ch.st.host["src"] = [np.ascontiguousarray(p) for p in src]
            got = ch.st.result()
            mid, _, want = chain_expected(pred, src, cus, ref_LX, qp, True)
            for k in range(3):
                np.testing.assert_array_equal(got["rec"][k], want[k], err_msg="replayed plane %d" % k)
                np.testing.assert_array_equal(got["coeff"][k], mid["coeff"][k])
            np.testing.assert_array_equal(got["cus"].view(np.uint8), mid["cus"].view(np.uint8))
    finally:
        L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


def test_bad_arguments_write_nothing_and_an_empty_map_is_a_no_op(api):
    w, h = 128, 64
    src, pred, cus = frame_case(w, h, 900, 1)
    st = Staged(api, src, pred, cus, 30)
    L = st.L
    bad_size = api.ref_picture_table([(st.ptr("src", 0), st.ptr("src", 1), st.ptr("src", 2), w, w // 2)], w - 4, h)
    no_plane = api.ref_picture_table([(0, st.ptr("src", 1), st.ptr("src", 2), w, w // 2)], w, h)
    sl = api.inter_residual_params(30, 0, 0, 1, scaling_list=1)
    rcs = [st.call(table=None), st.call(y=None), st.call(u=None), st.call(v=None), st.call(cus=None), st.call(cy=None), st.call(cu=None), st.call(cv=None),
           st.call(prm=None), st.call(table=bad_size.ctypes.data), st.call(table=no_plane.ctypes.data), st.call(prm=sl.ctypes.data), st.call(sy=w - 1),
           st.call(sc=w // 2 - 1), st.call(cy=st.ptr("coeff", 0) + 2)]
    for rc in rcs:
        assert rc == -2 and b"kvz_hip_inter_residual_frame" in L.kvz_hip_last_error()
    L.kvz_hip_stream_sync(None)
    got = st.result()
    init = RC.initial_outputs(w, h)
    untouched = {"rec": pred, "coeff": init[0], "cus": cus, "cbf_out": init[1], "costs": init[2]}
    RC.assert_outputs_equal(got, untouched, "after refused calls")
    assert L.kvz_hip_abi_version() == 4
    # optional outputs may be NULL; 4:0:0 needs no chroma pointer
    assert st.call(cbf=None, costs=None) == 0
    mono = Staged(api, (src[0], None, None), (pred[0], None, None), cus, 30, chroma=0)
    assert mono.call(u=None, v=None, cu=None, cv=None) == 0
    L.kvz_hip_stream_sync(None)
    # an all-intra and an all-blank map: nothing changes
    for typ in (IC.CU_INTRA, 0):
        none = np.array(cus)
        none["type"] = typ
        RC.assert_outputs_equal(run(api, src, pred, none, 30), {"rec": pred, "coeff": init[0], "cus": none, "cbf_out": init[1], "costs": init[2]},
                                "map of type %d" % typ)

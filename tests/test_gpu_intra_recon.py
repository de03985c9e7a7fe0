"""GPU: kvz_hip_intra_recon_frame against the committed fixture, against the composition of the reference's own functions in coding
order (tests/intra_recon_cases.py) on maps that stress the order between TUs, LCUs and wavefronts, and in the chain
kvz_hip_inter_recon_frame -> kvz_hip_inter_residual_frame -> kvz_hip_intra_recon_frame -> kvz_hip_deblock_frame -> kvz_hip_sao_frame on
one stream, eager and replayed from a captured graph.  Every output starts poisoned, every array is staged between guard bands, every
comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import inter_recon_cases as IC
import inter_residual_cases as RC
import intra_recon_cases as XC
import oracle_lib as O
import sao_frame_cases as SC
import test_gpu_inter_residual as TR
from patterns import CU_INFO, deblock_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra_recon.npz")


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


class Staged(TR.Staged):
    """the staging of the inter stage's test plus the modes; call() is the intra entry, inter_call() the inter one on the same arrays"""

    def __init__(self, A, src, rec, cus, modes, qp, chroma=1, signhide=0, slice_is_intra=0, init=None, scaling_list=0):
        TR.Staged.__init__(self, A, src, rec, cus, qp, chroma, signhide, slice_is_intra, init, scaling_list)
        self.host["modes"] = [np.ascontiguousarray(modes, dtype=np.uint8)]
        self.dev["modes"] = [self._up(self.host["modes"][0])]

    def args(self, over):
        a = {"table": self.table.ctypes.data, "y": self.ptr("rec", 0), "sy": self.host["rec"][0].shape[1], "u": self.ptr("rec", 1), "v": self.ptr("rec", 2),
             "sc": self.host["rec"][1].shape[1] if self.chroma else 0, "cus": self.ptr("cus"), "modes": self.ptr("modes"), "cy": self.ptr("coeff", 0),
             "cu": self.ptr("coeff", 1), "cv": self.ptr("coeff", 2), "cbf": self.ptr("cbf_out"), "costs": self.ptr("costs"), "prm": self.prm.ctypes.data}
        a.update(over)
        return a

    def call(self, stream=None, **over):
        a = self.args(over)
        return self.L.kvz_hip_intra_recon_frame(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["modes"], a["cy"], a["cu"], a["cv"],
                                                a["cbf"], a["costs"], a["prm"], stream)

    def inter_call(self, stream=None):
        return TR.Staged.call(self, stream)

    def result(self):
        np.testing.assert_array_equal(self.raw("modes", 0)[TR.GUARD:-TR.GUARD], self.host["modes"][0].reshape(-1), err_msg="the modes were written")
        return TR.Staged.result(self)


def run(A, src, rec, cus, modes, qp, chroma=1, signhide=0, slice_is_intra=0, **kw):
    from kvazaar_amd import _lib
    st = Staged(A, src, rec, cus, modes, qp, chroma, signhide, slice_is_intra, **kw)
    _lib.check(st.call(), "intra_recon_frame")
    _lib.check(st.L.kvz_hip_stream_sync(None), "sync")
    return st.result()


def test_every_output_equals_the_committed_fixture(api):
    z = np.load(GOLDEN, allow_pickle=False)
    for pic in XC.FIXTURE_PICTURES:
        name, w, h, chroma, qp, signhide, slice_is_intra = pic[:7]
        src, rec, cus, modes, want = XC.load_fixture_case(z, name, chroma)
        XC.assert_outputs_equal(run(api, src, rec, cus, modes, qp, chroma, signhide, slice_is_intra), want, name, chroma)
        # the numpy convenience, over zeroed outputs: the same inside the intra CUs
        conv = api.intra_recon_frame(src, rec, cus, modes, qp, chroma, signhide, slice_is_intra)
        zero = XC.compose(src, rec, cus, modes, qp, chroma, signhide, slice_is_intra)
        XC.assert_outputs_equal(conv, zero, name + " convenience", chroma)


def uniform_case(w, h, tu, seed):
    """an all-intra picture of TUs `tu` wide whose modes alternate 34 / 2 / 18: they pull across the top-right, the bottom-left and the
    corner, so that an ordering or visibility error between TUs, LCUs or wavefronts shows"""
    cus = np.zeros((h // 4, w // 4), dtype=CU_INFO)
    cus["type"] = IC.CU_INTRA
    if tu == 4:
        cus["depth"], cus["tr_depth"], cus["part_size"] = 3, 4, XC.SIZE_NXN
    else:
        cus["depth"] = cus["tr_depth"] = {32: 1, 16: 2, 8: 3}[tu]
    yy, xx = np.mgrid[0:h // 4, 0:w // 4]
    unit = tu // 4
    luma = np.array([34, 2, 18], np.uint8)[(xx // unit + 2 * (yy // unit)) % 3]
    step = max(unit, 2)
    modes = np.stack([luma, luma[(yy // step) * step, (xx // step) * step]], axis=-1)
    src, rec = XC.make_planes(cus, seed, 1, amps=(0, 2, 6, 12, 30))
    return src, rec, cus, modes


@pytest.mark.parametrize("tu", [4, 32])
def test_all_intra_picture_of_one_tu_size_equals_the_composition(api, tu):
    w, h, qp = 256, 192, 30
    src, rec, cus, modes = uniform_case(w, h, tu, 40 + tu)
    init = RC.initial_outputs(w, h, 1)
    want = XC.compose(src, rec, cus, modes, qp, 1, 1, 1, B=O, init=init)
    assert {t[1] for t in want["tus"] if t[0] == 0} == {tu} and {t[3] for t in want["tus"]} == {34, 2, 18} and any(t[2] for t in want["tus"])
    XC.assert_outputs_equal(run(api, src, rec, cus, modes, qp, 1, 1, 1, init=init), want, "all %dx%d" % (tu, tu))


def mixed_case(w, h, seed, chroma=1, pad=0, intra_share=0.35):
    cus, _, modes = XC.make_map(w, h, seed, intra_share=intra_share, blank_share=0.08)
    src, rec = XC.make_planes(cus, seed + 1, chroma, pad=pad)
    return src, rec, cus, modes


def test_what_the_intra_cus_held_on_entry_does_not_matter(api):
    w, h, qp = 200, 136, 27
    src, rec, cus, modes = mixed_case(w, h, 1000)
    other = XC.poison_intra(rec, cus, 1001)
    assert not np.array_equal(other[0], rec[0])
    a = run(api, src, rec, cus, modes, qp, 1, 1)
    b = run(api, src, other, cus, modes, qp, 1, 1)
    XC.assert_outputs_equal(a, b, "two poisons")
    XC.assert_outputs_equal(a, XC.compose(src, rec, cus, modes, qp, 1, 1, 0, B=O, init=RC.initial_outputs(w, h)), "against the composition")


@pytest.mark.parametrize("chroma", [1, 0])
def test_everything_outside_the_intra_cus_is_untouched(api, chroma):
    w, h, pad = 200, 136, 12
    src, rec, cus, modes = mixed_case(w, h, 1100, chroma, pad=pad)
    got = run(api, src, rec, cus, modes, 30, chroma, 0)
    m, mc, ms = XC.intra_mask(cus, w, h)
    assert m.any() and not m.all() and (cus["type"] == IC.CU_INTER).any() and (cus["type"] == 0).any()
    for k in range(3 if chroma else 1):
        mk, pw = (mc, w // 2) if k else (m, w)
        assert (got["rec"][k][:, pw:] == RC.POISON_PIXEL).all(), "wrote between width and stride"
        np.testing.assert_array_equal(got["rec"][k][:, :pw][~mk], rec[k][:, :pw][~mk])
        assert not np.array_equal(got["rec"][k][:, :pw][mk], rec[k][:, :pw][mk])
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
                    assert (c[lcu, z:z + 16] != RC.POISON_COEFF).all() if inside else (c[lcu, z:z + 16] == RC.POISON_COEFF).all(), \
                        "coefficients of LCU %d block (%d, %d)" % (lcu, bx, by)
    assert (got["cbf_out"][~ms] == RC.POISON_CBF).all() and (got["cbf_out"][ms] <= (7 if chroma else 1)).all()
    tl = np.zeros(ms.shape, bool)
    for (x, y, s) in XC.intra_cus(cus, w, h):
        tl[y // 4, x // 4] = True
    assert (got["costs"].view(np.uint32).reshape(ms.shape + (6,))[~tl] == RC.POISON_COST).all()
    assert (got["costs"].view(np.uint32).reshape(ms.shape + (6,))[tl] != RC.POISON_COST).all()
    # the records: nothing but cbf_y of the intra CUs changed
    before, after = np.array(cus), np.array(got["cus"])
    np.testing.assert_array_equal(after[~ms].view(np.uint8), before[~ms].view(np.uint8))
    before["cbf_y"], after["cbf_y"] = 0, 0
    np.testing.assert_array_equal(after.view(np.uint8), before.view(np.uint8))
    XC.assert_outputs_equal(got, XC.compose(src, rec, cus, modes, 30, chroma, 0, 0, B=O, init=RC.initial_outputs(w, h, chroma)), "padded", chroma)


@pytest.mark.parametrize("geom", [((2, 8, 220), (1, 4, 124), (1, 4, 124)), ((2, 3, 221), (1, 1, 125), (3, 7, 125))], ids=["aligned", "odd"])
def test_padded_strides_and_offset_bases_on_the_ragged_picture(api, geom):
    """planes inside larger buffers, per plane (rows above, columns left, stride): stride_c != stride_y / 2; bases 4-byte aligned but
    neither at the start of a row nor of the buffer, and odd bases with odd strides (PLANES in kvz_hip.h: any alignment)"""
    z = np.load(GOLDEN, allow_pickle=False)
    name, w, h, chroma, qp, signhide, slice_is_intra = XC.FIXTURE_PICTURES[0][:7]
    assert (name, w, h) == ("ragged", 200, 136)
    src, rec, cus, modes, want = XC.load_fixture_case(z, name, chroma)
    assert geom[1][2] != geom[0][2] // 2 and geom[1][2] == geom[2][2]
    big_rec, big_src = [], []
    for k, (top, left, stride) in enumerate(geom):
        ph, pw = rec[k].shape
        for planes, out in ((rec, big_rec), (src, big_src)):
            b = np.full((ph + max(g[0] for g in geom) + 2, stride), RC.POISON_PIXEL, np.uint8)
            b[top:top + ph, left:left + pw] = planes[k]
            out.append(b)
    st = Staged(api, big_src, big_rec, cus, modes, qp, chroma, signhide, slice_is_intra, init=RC.initial_outputs(w, h, chroma))
    off = [top * stride + left for (top, left, stride) in geom]
    table = api.ref_picture_table([(st.ptr("src", 0) + off[0], st.ptr("src", 1) + off[1], st.ptr("src", 2) + off[2], geom[0][2], geom[1][2])], w, h)
    from kvazaar_amd import _lib
    _lib.check(st.call(table=table.ctypes.data, y=st.ptr("rec", 0) + off[0], u=st.ptr("rec", 1) + off[1], v=st.ptr("rec", 2) + off[2],
                       sy=geom[0][2], sc=geom[1][2]), "intra_recon_frame")
    _lib.check(st.L.kvz_hip_stream_sync(None), "sync")
    got = st.result()
    planes = []
    for k, (top, left, stride) in enumerate(geom):
        ph, pw = rec[k].shape
        buf = got["rec"][k]
        planes.append(buf[top:top + ph, left:left + pw])
        outside = np.ones(buf.shape, bool)
        outside[top:top + ph, left:left + pw] = False
        assert (buf[outside] == RC.POISON_PIXEL).all(), "plane %d: wrote outside the picture" % k
    got["rec"] = tuple(planes)
    XC.assert_outputs_equal(got, want, "offset planes")


def test_refused_arguments_write_nothing(api):
    w, h = 128, 64
    src, rec, cus, modes = mixed_case(w, h, 1200)
    st = Staged(api, src, rec, cus, modes, 30)
    L = st.L
    bad_size = api.ref_picture_table([(st.ptr("src", 0), st.ptr("src", 1), st.ptr("src", 2), w, w // 2)], w - 4, h)
    sl = api.inter_residual_params(30, 0, 0, 1, scaling_list=1)
    rcs = [st.call(modes=None), st.call(cus=st.ptr("cus") + 2), st.call(cy=st.ptr("coeff", 0) + 2), st.call(cu=st.ptr("coeff", 1) + 8),
           st.call(table=bad_size.ctypes.data), st.call(sy=w - 1), st.call(sc=w // 2 - 1), st.call(prm=sl.ctypes.data), st.call(table=None), st.call(y=None),
           st.call(u=None), st.call(cus=None), st.call(cv=None), st.call(prm=None)]
    for rc in rcs:
        assert rc == -2 and b"kvz_hip_intra_recon_frame" in L.kvz_hip_last_error()
    L.kvz_hip_stream_sync(None)
    init = RC.initial_outputs(w, h)
    XC.assert_outputs_equal(st.result(), {"rec": rec, "coeff": init[0], "cus": cus, "cbf_out": init[1], "costs": init[2]}, "after refused calls")
    assert L.kvz_hip_abi_version() == 4
    # optional outputs may be NULL; 4:0:0 needs no chroma pointer; a map without intra CUs is a no-op
    assert st.call(cbf=None, costs=None) == 0
    mono = Staged(api, (src[0], None, None), (rec[0], None, None), cus, modes, 30, chroma=0)
    assert mono.call(u=None, v=None, cu=None, cv=None) == 0
    L.kvz_hip_stream_sync(None)
    none = np.array(cus)
    none["type"][none["type"] == IC.CU_INTRA] = 0
    XC.assert_outputs_equal(run(api, src, rec, none, modes, 30), {"rec": rec, "coeff": init[0], "cus": none, "cbf_out": init[1], "costs": init[2]},
                            "a map without intra CUs")


def test_full_hd_mixed_picture_equals_the_composed_oracle(api):
    """1920x1080: 30 x 17 LCUs with a ragged last row, 62 wavefronts; every output, every element"""
    w, h, qp = 1920, 1080, 32
    src, rec, cus, modes = mixed_case(w, h, 1300, intra_share=0.15)
    m, _, _ = XC.intra_mask(cus, w, h)
    assert 0.08 < m.mean() < 0.25
    init = RC.initial_outputs(w, h, 1)
    want = XC.compose(src, rec, cus, modes, qp, 1, 1, 0, B=O, init=init)
    assert {t[1] for t in want["tus"] if t[0] == 0} == {4, 8, 16, 32}
    XC.assert_outputs_equal(run(api, src, rec, cus, modes, qp, 1, 1, 0, init=init), want, "1080p")


def test_malformed_map_completes_inside_the_arrays(api):
    """modes of 35 and 255, intra records of depth 7, SCUs of one CU that disagree: the content is unspecified; the call completes, the
    guard bands (checked by result()) and the bytes between width and stride are intact"""
    w, h = 200, 136
    g = np.random.default_rng(17)
    cus = np.zeros((h // 4, w // 4), dtype=CU_INFO)
    cus["type"] = g.integers(0, 3, cus.shape)
    cus["depth"] = g.choice([0, 1, 2, 3, 3, 7], cus.shape)
    cus["tr_depth"] = g.integers(0, 256, cus.shape)
    cus["part_size"] = g.integers(0, 9, cus.shape)
    modes = g.choice(np.array([0, 1, 2, 10, 26, 34, 35, 255], np.uint8), cus.shape + (2,))
    assert ((cus["type"] == IC.CU_INTRA) & (cus["depth"] == 7)).any() and (modes == 35).any() and (modes == 255).any()
    rec = RC.smooth_planes(w, h, 18, 1, pad=20)
    src = RC.smooth_planes(w, h, 19, 1)
    got = run(api, src, rec, cus, modes, 26, 1, 1)
    for k in range(3):
        assert (got["rec"][k][:, (w >> (1 if k else 0)):] == RC.POISON_PIXEL).all()


def chain_case(w, h, seed, n_refs, ref_LX=None):
    refs = IC.random_planes(w, h, seed, n_refs)
    cus, own_LX, modes = XC.make_map(w, h, seed + 1, intra_share=0.3, blank_share=0.0, n_refs=n_refs, slice_b=True, bad_share=0.0, edge_cu=False)
    ref_LX = own_LX if ref_LX is None else ref_LX
    dest = tuple(np.full((h >> (1 if k else 0), w >> (1 if k else 0)), RC.POISON_PIXEL, np.uint8) for k in range(3))
    pred = IC.compose(refs, IC.walk_pus(cus, ref_LX, w, h), (h, w), 1, dest)
    inter_src = RC.make_source(pred, cus, seed + 2, 1)
    intra_src, _ = XC.make_planes(cus, seed + 3, 1)
    m, mc, _ = XC.intra_mask(cus, w, h)
    src = tuple(np.where(mc if k else m, intra_src[k], inter_src[k]).astype(np.uint8) for k in range(3))
    return refs, cus, modes, ref_LX, dest, pred, src


def chain_expected(pred, src, cus, modes, ref_LX, qp, sao):
    mid = RC.compose(src, pred, cus, qp, 1, 0, many=True)
    full = XC.compose(src, mid["rec"], mid["cus"], modes, qp, 1, 0, 0, B=O, init=(mid["coeff"], mid["cbf_out"], mid["costs"]))
    prm = deblock_params(qp=qp, slice_is_b=1, chroma=1)
    prm["ref_LX"] = ref_LX
    deb = O.deblock_frame(full["rec"][0], full["rec"][1], full["rec"][2], full["cus"], prm)
    return full, deb, SC.compose_recon(deb, sao[0], sao[1], 1)


class Chain:
    """the five calls on device arrays that stay put"""

    def __init__(self, A, case, qp, sao):
        from kvazaar_amd import _lib
        refs, cus, modes, ref_LX, dest, pred, src = case
        self.A, self.L, self.check = A, _lib.init(0), _lib.check
        self.h, self.w = src[0].shape
        self.recon = A._Recon(refs, (self.h, self.w), 1, dest)
        zero = (tuple(np.zeros_like(c) for c in RC.initial_outputs(self.w, self.h)[0]), np.zeros(cus.shape, np.uint8), np.zeros(cus.shape, RC.COST))
        self.st = Staged(A, src, dest, cus, modes, qp, 1, 0, init=zero)
        self.rprm = np.zeros(1, dtype=A.INTER_RECON_PARAMS)
        self.rprm["chroma"], self.rprm["n_refs"], self.rprm["ref_LX"] = 1, len(refs), ref_LX
        self.dprm = deblock_params(qp=qp, slice_is_b=1, chroma=1)
        self.dprm["ref_LX"] = ref_LX
        self.sao = [A.DeviceBuffer.from_numpy(np.ascontiguousarray(r, dtype=np.int32)) for r in sao]
        self.out = [A.DeviceBuffer.from_numpy(np.full_like(p, RC.POISON_PIXEL)) for p in dest]

    def launch(self, s):
        st, w, h = self.st, self.w, self.h
        y, u, v = st.ptr("rec", 0), st.ptr("rec", 1), st.ptr("rec", 2)
        self.check(self.L.kvz_hip_inter_recon_frame(y, w, u, v, w // 2, w, h, st.ptr("cus"), self.recon.table.ctypes.data, self.rprm.ctypes.data, s),
                   "inter_recon_frame")
        self.check(st.inter_call(s), "inter_residual_frame")
        self.check(st.call(s), "intra_recon_frame")
        self.check(self.L.kvz_hip_deblock_frame(y, w, u, v, w // 2, w, h, st.ptr("cus"), self.dprm.ctypes.data, s), "deblock_frame")
        self.check(self.L.kvz_hip_sao_frame(y, w, u, v, w // 2, self.out[0].ptr, w, self.out[1].ptr, self.out[2].ptr, w // 2, w, h, self.sao[0].ptr,
                                            self.sao[1].ptr, 1, s), "sao_frame")

    def compare(self, want, what):
        full, deb, sao = want
        got = self.st.result()
        for k in range(3):
            np.testing.assert_array_equal(got["rec"][k], deb[k], err_msg="%s: plane %d after deblocking" % (what, k))
            np.testing.assert_array_equal(got["coeff"][k], full["coeff"][k], err_msg="%s: coefficients %d" % (what, k))
            np.testing.assert_array_equal(self.out[k].to_numpy(np.uint8, sao[k].shape), sao[k], err_msg="%s: plane %d after SAO" % (what, k))
        np.testing.assert_array_equal(got["cus"].view(np.uint8), full["cus"].view(np.uint8), err_msg=what)
        np.testing.assert_array_equal(got["cbf_out"], full["cbf_out"], err_msg=what)
        np.testing.assert_array_equal(got["costs"].view(np.uint32), full["costs"].view(np.uint32), err_msg=what)


def test_five_stage_chain_on_one_stream_and_replayed_from_a_graph(api):
    w, h, qp, n_refs = 256, 192, 30, 2
    first = chain_case(w, h, 1400, n_refs)
    second = chain_case(w, h, 1410, n_refs, ref_LX=first[3])            # params are copied at capture: the first picture's ref_LX
    sao = (SC.make_records(w, h, 1420, 0), SC.make_records(w, h, 1421, 1))
    ch = Chain(api, first, qp, sao)
    L, s, graph = ch.L, ch.L.kvz_hip_stream_create(), C.c_void_p()
    try:
        ch.launch(s)                                                    # five asynchronous calls, nothing between them
        ch.check(L.kvz_hip_stream_sync(s), "sync")
        ch.compare(chain_expected(first[5], first[6], first[1], first[2], first[3], qp, sao), "eager")
        ch.check(L.kvz_hip_graph_begin(s), "graph_begin")
        ch.launch(s)
        ch.check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        for n, (refs, cus, modes, ref_LX, dest, pred, src) in enumerate((second, first)):
            for i, r in enumerate(refs):
                for k in range(3):
                    a = np.ascontiguousarray(r[k])
                    ch.check(L.kvz_hip_memcpy_h2d(ch.recon.keep[3 * i + k].ptr, a.ctypes.data, a.nbytes, s), "h2d")
            for k in range(3):
                ch.st.upload("src", k, src[k], s)
                ch.st.upload("rec", k, dest[k], s)
                ch.st.upload("coeff", k, np.zeros_like(ch.st.host["coeff"][k]), s)
            ch.st.upload("cus", 0, cus, s)
            ch.st.upload("modes", 0, modes, s)
            ch.st.upload("cbf_out", 0, np.zeros_like(ch.st.host["cbf_out"][0]), s)
            ch.st.upload("costs", 0, np.zeros_like(ch.st.host["costs"][0]), s)
            ch.check(L.kvz_hip_stream_sync(s), "sync")
            ch.check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            ch.check(L.kvz_hip_stream_sync(s), "sync")
            ch.st.host["src"] = [np.ascontiguousarray(p) for p in src]
            ch.st.host["modes"] = [np.ascontiguousarray(modes)]
            ch.compare(chain_expected(pred, src, cus, modes, ref_LX, qp, sao), "replay %d" % n)
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)

"""GPU: the lossless entries of the picture chain -- kvz_hip_inter_residual_frame_lossless and kvz_hip_intra_recon_frame_lossless --
against the committed fixture (tests/lossless_cases.py: reference pixels and predictions from the reference's own functions, bypass and
DPCM restated and pinned on the CPU); over poisoned outputs and poisoned rec planes; on padded, offset and unequal strides; with and
without a tile grid and tile by tile; replayed from a captured graph after every input changed; for what they refuse; against the
composition on random maps and on an all-4x4 picture.  Every array is staged between guard bands, every comparison is exact.  Every test
runs under a time limit of its own that ends the process, and after a call or a synchronisation that reports a runtime error no further
test starts anything on the device."""
import ctypes as C
import faulthandler
import os
import sys

import numpy as np
import pytest

import inter_recon_cases as IC
import inter_residual_cases as RC
import intra_recon_cases as XC
import lossless_cases as LC
import tile_chain_cases as TC
from patterns import CU_INFO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lossless.npz")
GUARD, GUARD_BYTE = 512, 0xC3
INVALID = -2
PICS = {p[0]: p for p in LC.FIXTURE_PICTURES}
TEST_LIMIT_S = 60                                                     # every test takes a fraction of a second
FAULTS = []


def check(rc, what):
    from kvazaar_amd import _lib
    try:
        _lib.check(rc, what)
    except Exception:
        FAULTS.append(what)
        raise


@pytest.fixture(autouse=True)
def limits():
    assert not FAULTS, "an earlier test met a device error (%s): nothing more is started" % FAULTS[0]
    faulthandler.dump_traceback_later(TEST_LIMIT_S, exit=True, file=sys.__stderr__)
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


def padded(plane, pad):
    a = np.full((plane.shape[0], plane.shape[1] + pad), RC.POISON_PIXEL, np.uint8)
    a[:, :plane.shape[1]] = plane
    return a


class Staged:
    """every array of the two calls in device memory between guard bands.  The rec planes start as the case's prediction (or `rec`).
    src_pad / rec_pad: (luma, chroma) extra columns = strides beyond the widths; offset: the planes and cbf_out begin that many bytes
    into their buffers (an odd base address).  Outputs start poisoned (RC.initial_outputs) unless init is given."""

    def __init__(self, A, case, implicit_rdpcm=0, init=None, rec=None, src_pad=(0, 0), rec_pad=(0, 0), offset=0, grid="case"):
        from kvazaar_amd import _lib
        self.A, self.L, self.B = A, _lib.init(0), _lib
        self.chroma, self.n = int(case["chroma"]), 3 if case["chroma"] else 1
        self.w, self.h = case["width"], case["height"]
        self.offset = offset
        init = init or RC.initial_outputs(self.w, self.h, self.chroma)
        rec = rec or case["pred"]
        self.host = {"src": [padded(p, src_pad[k > 0]) for k, p in enumerate(case["src"][:self.n])],
                     "rec": [padded(p[:self.h >> (k > 0), :self.w >> (k > 0)], rec_pad[k > 0]) for k, p in enumerate(rec[:self.n])],
                     "coeff": [np.ascontiguousarray(c) for c in init[0][:self.n]], "cus": [np.ascontiguousarray(case["cus"])],
                     "modes": [np.ascontiguousarray(case["modes"], dtype=np.uint8)],
                     "cbf_out": [np.ascontiguousarray(init[1])], "costs": [np.ascontiguousarray(init[2])]}
        self.off = {k: (offset if k in ("src", "rec", "cbf_out", "modes") else 0) for k in self.host}
        self.dev = {k: [self._up(a, self.off[k]) for a in v] for k, v in self.host.items()}
        self.ll = _lib.Lossless(self.chroma, int(implicit_rdpcm), (0, 0))
        self.table = A.ref_picture_table([(self.ptr("src", 0), self.ptr("src", 1) or 0, self.ptr("src", 2) or 0, self.host["src"][0].shape[1],
                                           self.host["src"][1].shape[1] if self.chroma else 0)], self.w, self.h)
        grid = case["grid"] if grid == "case" else grid
        self.grid = A.tile_grid(self.w, self.h, *grid) if grid else None

    def _up(self, a, off):
        raw = np.full(a.nbytes + 2 * GUARD + off, GUARD_BYTE, np.uint8)
        raw[GUARD + off:GUARD + off + a.nbytes] = a.view(np.uint8).reshape(-1)
        return self.A.DeviceBuffer.from_numpy(raw)

    def ptr(self, kind, k=0):
        return self.dev[kind][k].ptr + GUARD + self.off[kind] if k < len(self.dev[kind]) else None

    def upload(self, kind, k, a, stream=None):
        a = np.ascontiguousarray(a)
        assert a.nbytes == self.host[kind][k].nbytes
        check(self.L.kvz_hip_memcpy_h2d(self.ptr(kind, k), a.ctypes.data, a.nbytes, stream), "h2d")
        self._keep = getattr(self, "_keep", []) + [a]

    def args(self, over):
        a = {"table": self.table.ctypes.data, "y": self.ptr("rec", 0), "sy": self.host["rec"][0].shape[1], "u": self.ptr("rec", 1), "v": self.ptr("rec", 2),
             "sc": self.host["rec"][1].shape[1] if self.chroma else 0, "cus": self.ptr("cus"), "modes": self.ptr("modes"), "cy": self.ptr("coeff", 0),
             "cu": self.ptr("coeff", 1), "cv": self.ptr("coeff", 2), "cbf": self.ptr("cbf_out"), "costs": self.ptr("costs"),
             "grid": self.grid.ctypes.data if self.grid is not None else None, "ll": C.byref(self.ll)}
        a.update(over)
        return a

    def inter(self, stream=None, **over):
        a = self.args(over)
        return self.L.kvz_hip_inter_residual_frame_lossless(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["cy"], a["cu"], a["cv"],
                                                            a["cbf"], a["costs"], a["ll"], stream)

    def intra(self, stream=None, **over):
        a = self.args(over)
        return self.L.kvz_hip_intra_recon_frame_lossless(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["modes"], a["cy"], a["cu"],
                                                         a["cv"], a["cbf"], a["costs"], a["grid"], a["ll"], stream)

    def sync(self, stream=None):
        check(self.L.kvz_hip_stream_sync(stream), "sync")

    def result(self):
        """-> the outputs as LC.compose returns them, the planes cut to the picture; asserts every guard band, the columns beyond the
        widths and that the source and the modes were not written"""
        out = {}
        for kind in self.dev:
            got = []
            for k, a in enumerate(self.host[kind]):
                raw = self.dev[kind][k].to_numpy(np.uint8, (a.nbytes + 2 * GUARD + self.off[kind],))
                lead = GUARD + self.off[kind]
                assert (raw[:lead] == GUARD_BYTE).all() and (raw[lead + a.nbytes:] == GUARD_BYTE).all(), "guard band of %s %d" % (kind, k)
                got.append(raw[lead:lead + a.nbytes].view(a.dtype).reshape(a.shape))
            out[kind] = got
        for kind in ("src", "modes"):
            for g, a in zip(out[kind], self.host[kind]):
                np.testing.assert_array_equal(g, a, err_msg="%s was written" % kind)
        rec = []
        for k, g in enumerate(out["rec"]):
            pw = self.w >> (k > 0)
            assert (g[:, pw:] == RC.POISON_PIXEL).all(), "the columns beyond the width of rec %d" % k
            rec.append(g[:, :pw])
        pad = [None] * (3 - self.n)
        return {"rec": tuple(rec + pad), "coeff": tuple(out["coeff"] + pad), "cus": out["cus"][0], "cbf_out": out["cbf_out"][0], "costs": out["costs"][0]}


def run_both(st, stream=None):
    check(st.inter(stream), "inter_residual_frame_lossless")
    check(st.intra(stream), "intra_recon_frame_lossless")


def ran(api, case, r, **kw):
    st = Staged(api, case, r, **kw)
    run_both(st)
    st.sync()
    return st.result()


# ---------------------------------------------------------------- 1. the fixture, entry by entry
@pytest.mark.parametrize("rdpcm", [0, 1])
@pytest.mark.parametrize("name", list(PICS))
def test_fixture_through_both_entries(api, golden, name, rdpcm):
    case = LC.load_case(golden, PICS[name])
    chroma = case["chroma"]
    st = Staged(api, case, rdpcm)
    check(st.inter(), "inter_residual_frame_lossless")
    st.sync()
    mid = LC.load_want(golden, name, "mid", chroma)                  # implicit_rdpcm does not touch inter CUs
    LC.assert_outputs_equal(st.result(), mid, "%s inter" % name, chroma)
    check(st.intra(), "intra_recon_frame_lossless")
    st.sync()
    if rdpcm in case["rdpcm"]:
        want = LC.load_want(golden, name, "full%d" % rdpcm, chroma)
    elif not case["rdpcm"]:
        want = mid                                                   # no intra CU: nothing more happens
    else:
        want = LC.compose(case, rdpcm)[1]
    LC.assert_outputs_equal(st.result(), want, "%s intra" % name, chroma)


def test_numpy_conveniences_route_to_the_entries(api, golden):
    for name in ("mixed", "mono"):
        case = LC.load_case(golden, PICS[name])
        chroma, w, h = case["chroma"], case["width"], case["height"]
        init = RC.initial_outputs(w, h, chroma)
        mid = api.inter_residual_frame_lossless(case["src"], case["pred"], case["cus"], chroma, 1, coeff=init[0], cbf_out=init[1], costs=init[2])
        LC.assert_outputs_equal(mid, LC.load_want(golden, name, "mid", chroma), name + " inter convenience", chroma)
        tiles = api.tile_grid(w, h, *case["grid"]) if case["grid"] else None
        full = api.intra_recon_frame_lossless(case["src"], mid["rec"], mid["cus"], case["modes"], chroma, 1, tiles, coeff=mid["coeff"],
                                              cbf_out=mid["cbf_out"], costs=mid["costs"])
        LC.assert_outputs_equal(full, LC.load_want(golden, name, "full1", chroma), name + " intra convenience", chroma)


# ---------------------------------------------------------------- 2. poison stays outside the entries' own CUs and TUs
def test_poison_survives_outside_the_own_cus_and_tus(api, golden):
    """worked out from the map alone, not from the fixture's outputs"""
    case = LC.load_case(golden, PICS["mixed"])
    w, h = case["width"], case["height"]
    got = ran(api, case, 1)
    owned, first = np.zeros(case["cus"].shape, bool), np.zeros(case["cus"].shape, bool)
    for (x, y, s) in RC.inter_cus(case["cus"], w, h) + XC.intra_cus(case["cus"], w, h):
        owned[y // 4:(y + s) // 4, x // 4:(x + s) // 4] = True
        first[y // 4, x // 4] = True
    assert (~owned).any() and (got["cbf_out"][~owned] == RC.POISON_CBF).all() and (got["cbf_out"][owned] <= 7).all()
    assert (got["costs"].view(np.uint32).reshape(first.shape + (6,))[~first] == RC.POISON_COST).all()
    np.testing.assert_array_equal(got["cus"][~owned].view(np.uint8), case["cus"][~owned].view(np.uint8))
    covered = [np.zeros((6, 4096), bool), np.zeros((6, 1024), bool), np.zeros((6, 1024), bool)]
    pixels = [np.zeros((h >> (k > 0), w >> (k > 0)), bool) for k in range(3)]
    tus = [(t[0], t[1], t[2], t[3]) for t in RC.walk_tus(case["cus"], w, h, 1)]
    for t in TC.tiles(w, h, *case["grid"]):
        tus += [(u[0], u[1] + t[0], u[2] + t[1], u[3]) for u in XC.walk_tus(TC.crop_map(case["cus"], t), TC.crop_map(case["modes"], t), t[2] - t[0], t[3] - t[1], 1)]
    for (p, x, y, n) in tus:
        sh = 1 if p else 0
        z = RC.xy_to_zorder(32 if p else 64, (x & 63) >> sh, (y & 63) >> sh)
        covered[p][(y >> 6) * 3 + (x >> 6), z:z + n * n] = True
        pixels[p][y >> sh:(y >> sh) + n, x >> sh:(x >> sh) + n] = True
    for p in range(3):
        assert (~covered[p]).any() and (got["coeff"][p][~covered[p]] == np.int16(RC.POISON_COEFF)).all(), p
        assert (got["rec"][p][~pixels[p]] == case["pred"][p][~pixels[p]]).all() and (got["rec"][p][pixels[p]] == case["src"][p][pixels[p]]).all(), p


# ---------------------------------------------------------------- 3. the intra entry reads the source only
@pytest.mark.parametrize("name", ["intra", "mixed"])
def test_intra_entry_never_reads_rec(api, golden, name):
    case = LC.load_case(golden, PICS[name])
    g = np.random.default_rng(7)
    want = LC.load_want(golden, name, "full1", 1)
    mid = LC.load_want(golden, name, "mid", 1)
    noise = tuple(g.integers(0, 256, p.shape).astype(np.uint8) for p in case["src"])
    st = Staged(api, dict(case, cus=mid["cus"]), 1, init=(mid["coeff"], mid["cbf_out"], mid["costs"]), rec=noise)
    check(st.intra(), "intra_recon_frame_lossless")
    st.sync()
    got = st.result()
    rec = []
    for k in range(3):
        # the pixels the entry writes: the intra CUs, but for a CU whose mode above 34 makes it skip the plane
        inside = np.zeros(case["src"][0].shape, bool)
        for (x, y, size) in XC.intra_cus(case["cus"], case["width"], case["height"]):
            inside[y:y + size, x:x + size] = case["modes"][y // 4, x // 4, 1 if k else 0] <= 34
        inside = inside[::2, ::2] if k else inside
        assert (got["rec"][k][~inside] == noise[k][~inside]).all(), "rec outside the intra CUs was written"
        rec.append(np.where(inside, got["rec"][k], want["rec"][k]))
    LC.assert_outputs_equal(dict(got, rec=tuple(rec)), want, name + " over noise", 1)


# ---------------------------------------------------------------- 4. the reconstruction is the source
def test_rec_equals_source_over_every_covered_cu(api, golden):
    case = LC.load_case(golden, PICS["mixed"])
    w, h = case["width"], case["height"]
    got = ran(api, case, 0)
    luma, chroma = np.zeros((h, w), bool), np.zeros((h, w), bool)
    for (x, y, s) in RC.inter_cus(case["cus"], w, h):
        luma[y:y + s, x:x + s] = chroma[y:y + s, x:x + s] = True
    for (x, y, s) in XC.intra_cus(case["cus"], w, h):                # but for the two CUs whose mode above 34 makes the entry skip a plane
        luma[y:y + s, x:x + s] = case["modes"][y // 4, x // 4, 0] <= 34
        chroma[y:y + s, x:x + s] = case["modes"][y // 4, x // 4, 1] <= 34
    assert luma.sum() > 0.8 * w * h and (got["rec"][0][luma] == case["src"][0][luma]).all()
    for k in (1, 2):
        assert (got["rec"][k][chroma[::2, ::2]] == case["src"][k][chroma[::2, ::2]]).all()


# ---------------------------------------------------------------- 5. the PLANES rule
@pytest.mark.parametrize("name", ["intra", "mixed"])
@pytest.mark.parametrize("layout", [dict(src_pad=(3, 3), rec_pad=(3, 3)), dict(offset=1), dict(src_pad=(8, 1), rec_pad=(5, 2), offset=3)])
def test_strides_and_offsets(api, golden, name, layout):
    """padded strides; odd base addresses; strides that differ between source, rec and chroma, on odd bases"""
    case = LC.load_case(golden, PICS[name])
    LC.assert_outputs_equal(ran(api, case, 1, **layout), LC.load_want(golden, name, "full1", 1), "%s %r" % (name, layout), 1)


# ---------------------------------------------------------------- 6, 7. tiles
def test_null_grid_is_one_tile(api, golden):
    case = LC.load_case(golden, PICS["mixed"])
    a = ran(api, case, 1, grid=None)
    b = ran(api, case, 1, grid=TC.one_tile(case["width"], case["height"]))
    LC.assert_outputs_equal(a, b, "NULL against one tile", 1)
    assert not np.array_equal(a["coeff"][0], LC.load_want(golden, "mixed", "full1", 1)["coeff"][0]), "the grid matters"


def test_each_tile_equals_the_untiled_entry_on_that_tile(api, golden):
    case = LC.load_case(golden, PICS["mixed"])
    w, h = case["width"], case["height"]
    whole = ran(api, case, 1, init=LC.RC.initial_outputs(w, h, 1))
    for t in TC.tiles(w, h, *case["grid"]):
        tw, th = t[2] - t[0], t[3] - t[1]
        sub = dict(case, width=tw, height=th, grid=None, src=TC.crop_planes(case["src"], t, 3), pred=TC.crop_planes(case["pred"], t, 3),
                   cus=TC.crop_map(case["cus"], t), modes=TC.crop_map(case["modes"], t))
        part = ran(api, sub, 1)
        for k in range(3):
            np.testing.assert_array_equal(part["rec"][k], TC.crop_planes(whole["rec"], t, 3)[k], err_msg="tile at %d,%d rec %d" % (t[0], t[1], k))
            np.testing.assert_array_equal(part["coeff"][k], whole["coeff"][k][t[4]], err_msg="tile at %d,%d coeff %d" % (t[0], t[1], k))
        np.testing.assert_array_equal(part["cus"].view(np.uint8), TC.crop_map(whole["cus"], t).view(np.uint8))
        np.testing.assert_array_equal(part["cbf_out"], TC.crop_map(whole["cbf_out"], t))
        np.testing.assert_array_equal(part["costs"].view(np.uint32), TC.crop_map(whole["costs"], t).view(np.uint32))


# ---------------------------------------------------------------- 8. capture
def test_captured_calls_replay_after_every_input_changed(api, golden):
    case = LC.load_case(golden, PICS["mixed"])
    other = dict(LC.fixture_case(("other", 136, 72, 1, 9001, 0.4, LC.TILED, (1,))), name="mixed")
    wants = {"first": LC.load_want(golden, "mixed", "full1", 1), "other": LC.compose(other, 1)[1]}
    assert not np.array_equal(other["cus"].view(np.uint8), case["cus"].view(np.uint8)) and not np.array_equal(other["src"][0], case["src"][0])
    st = Staged(api, case, 1)
    L, s, graph = st.L, st.L.kvz_hip_stream_create(), C.c_void_p()
    check(L.kvz_hip_graph_begin(s), "graph_begin")
    run_both(st, s)
    check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
    assert graph.value
    try:
        init = RC.initial_outputs(136, 72, 1)
        for which, c in (("first", case), ("other", other), ("first", case)):
            fresh = {"src": c["src"], "rec": c["pred"], "coeff": init[0], "cus": [c["cus"]], "modes": [c["modes"]], "cbf_out": [init[1]], "costs": [init[2]]}
            for kind, arrays in fresh.items():
                for k, a in enumerate(arrays):
                    st.upload(kind, k, a, s)
                    st.host[kind][k] = np.ascontiguousarray(a)
            st.sync(s)
            check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            st.sync(s)
            LC.assert_outputs_equal(st.result(), wants[which], "replayed on the %s picture" % which, 1)
            eager = ran(api, c, 1)
            LC.assert_outputs_equal(st.result(), eager, "replay against a fresh eager call (%s)" % which, 1)
    finally:
        L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


# ---------------------------------------------------------------- 9. refusals
def test_refusals_name_the_entry_and_write_nothing(api, golden):
    from kvazaar_amd import _lib
    case = LC.load_case(golden, PICS["mixed"])
    w, h = case["width"], case["height"]
    st = Staged(api, case, 1)
    L = st.L
    reserved = [_lib.Lossless(1, 1, (1, 0)), _lib.Lossless(1, 1, (0, -1))]
    table = lambda **kw: api.ref_picture_table([(kw.get("y", st.ptr("src", 0)), kw.get("u", st.ptr("src", 1)), kw.get("v", st.ptr("src", 2)), kw.get("sy", w),
                                                 kw.get("sc", w // 2))], kw.get("w", w), kw.get("h", h))
    tables = [table(w=w - 4), table(h=h + 4), table(sy=w - 1), table(sc=w // 2 - 1), table(y=0), table(u=0), table(v=0)]
    bad_grid = api.tile_grid(w, h, *case["grid"])
    bad_grid["col_bd"][0, 1] = 0
    short_grid = api.tile_grid(w, h, (0, 1, 2), (0, 1, 2))
    for call, entry in ((st.inter, b"kvz_hip_inter_residual_frame_lossless"), (st.intra, b"kvz_hip_intra_recon_frame_lossless")):
        overs = [{"ll": None}, {"ll": C.byref(reserved[0])}, {"ll": C.byref(reserved[1])}, {"table": None}, {"y": None}, {"u": None}, {"v": None},
                 {"cus": None}, {"cy": None}, {"cu": None}, {"cv": None}, {"cus": st.ptr("cus") + 2}, {"cy": st.ptr("coeff", 0) + 8},
                 {"cv": st.ptr("coeff", 2) + 2}, {"costs": st.ptr("costs") + 1}, {"sy": w - 1}, {"sc": w // 2 - 1}]
        overs += [{"table": t.ctypes.data} for t in tables]
        if call == st.intra:
            overs += [{"modes": None}, {"grid": bad_grid.ctypes.data}, {"grid": short_grid.ctypes.data}]
        for over in overs:
            assert call(**over) == INVALID, (entry, sorted(over))
            assert entry in L.kvz_hip_last_error(), (entry, sorted(over), L.kvz_hip_last_error())
    st.sync()
    init = RC.initial_outputs(w, h, 1)
    untouched = {"rec": case["pred"], "coeff": init[0], "cus": case["cus"], "cbf_out": init[1], "costs": init[2]}
    LC.assert_outputs_equal(st.result(), untouched, "after refused calls", 1)
    # the optional outputs may be missing
    check(st.inter(cbf=None, costs=None), "inter_residual_frame_lossless")
    check(st.intra(cbf=None, costs=None), "intra_recon_frame_lossless")
    st.sync()
    want = LC.load_want(golden, "mixed", "full1", 1)
    LC.assert_outputs_equal(st.result(), dict(want, cbf_out=init[1], costs=init[2]), "without cbf_out and costs", 1)
    assert L.kvz_hip_abi_version() == 4


# ---------------------------------------------------------------- 10. a seeded differential
DIFFERENTIAL = ((72, 72, 1, None), (136, 136, 1, ((0, 2, 3), (0, 1, 3))), (104, 88, 0, None), (136, 72, 1, ((0, 1, 3), (0, 2))), (72, 136, 0, ((0, 1, 2), (0, 2, 3))),
                (96, 120, 1, ((0, 1, 2), (0, 1, 2))), (120, 104, 1, None), (88, 128, 0, ((0, 2), (0, 1, 2))))


@pytest.mark.parametrize("i", range(len(DIFFERENTIAL)))
def test_random_quadtree_maps_equal_the_composition(api, i):
    w, h, chroma, grid = DIFFERENTIAL[i]
    cus, _, modes = XC.make_map(w, h, 4200 + i, intra_share=0.5, blank_share=0.1)
    g = np.random.default_rng(4300 + i)
    for (x, y, s) in XC.intra_cus(cus, w, h):                        # the DPCM modes, often
        if g.random() < 0.4:
            modes[y // 4:(y + s) // 4, x // 4:(x + s) // 4, int(g.integers(0, 2))] = (10, 26)[int(g.integers(0, 2))]
    src, pred = LC.make_planes(w, h, 4400 + i, chroma)
    case = {"name": "random", "width": w, "height": h, "chroma": chroma, "grid": grid, "src": src, "pred": pred, "cus": cus, "modes": modes}
    rdpcm = i % 2
    mid, full = LC.compose(case, rdpcm)
    assert len(mid["tus"]) > 10 and len(full["tus"]) > 10
    LC.assert_outputs_equal(ran(api, case, rdpcm), full, "random map %d" % i, chroma)


# ---------------------------------------------------------------- 11. the case the lossy wavefront exists for
def test_all_4x4_intra_picture(api):
    w, h = 136, 72
    cus = np.zeros((h // 4, w // 4), dtype=CU_INFO)
    cus["type"], cus["depth"], cus["tr_depth"], cus["part_size"] = IC.CU_INTRA, 3, 4, XC.SIZE_NXN
    g = np.random.default_rng(77)
    modes = g.choice((0, 1, 2, 10, 18, 26, 34, 7, 29), cus.shape + (2,)).astype(np.uint8)
    src, pred = LC.make_planes(w, h, 78, 1)
    case = {"name": "all4", "width": w, "height": h, "chroma": 1, "grid": None, "src": src, "pred": pred, "cus": cus, "modes": modes}
    for rdpcm in (0, 1):
        mid, full = LC.compose(case, rdpcm)
        assert not mid["tus"] and len(full["tus"]) == (w // 4) * (h // 4) + 2 * (w // 8) * (h // 8)
        LC.assert_outputs_equal(ran(api, case, rdpcm), full, "all 4x4, implicit_rdpcm %d" % rdpcm, 1)

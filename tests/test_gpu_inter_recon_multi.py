"""GPU: kvz_hip_inter_recon_frames -- motion compensation of up to sixteen pictures over one shared pool of reference pictures -- against
kvz_hip_inter_recon_frame called per picture with the table gathered from the pool (THE RULE of include/kvz_hip.h), against the committed
fixture tests/golden/inter_recon.npz, and through the chain into kvz_hip_inter_residual_frames and kvz_hip_deblock_frames.  Every
destination plane starts poisoned, every comparison is exact and covers the whole buffer, padding included."""
import ctypes as C
import faulthandler
import sys

import numpy as np
import pytest

import inter_recon_cases as IC
import inter_residual_cases as RC
from patterns import deblock_params
from test_gpu_inter_recon import GOLDEN, POISON, poisoned

pytestmark = pytest.mark.gpu

INVALID = -2
TEST_LIMIT_S = 60                                                     # every test takes a few seconds at the most
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


# ---------------------------------------------------------------- pictures and calls
def picture(w, h, refs, cus, ref_LX, chroma=1, dest=None):
    """one record: refs are pool indices, dest the initial destination planes (arrays or PlaneViews; default poison of the picture size)"""
    return {"width": w, "height": h, "chroma": chroma, "refs": list(refs), "cus": np.ascontiguousarray(cus), "ref_LX": np.array(ref_LX, dtype=np.uint8),
            "dest": dest if dest is not None else poisoned(w, h, chroma)}


def random_picture(w, h, seed, refs, slice_b=False, chroma=1, dest=None, **kw):
    cus, ref_LX = IC.random_cu_map(w, h, seed, len(refs), slice_b, **kw)
    return picture(w, h, refs, cus, ref_LX, chroma, dest)


GARBAGE = "garbage"                                                   # a pool slot that no record names: NULL planes, a size of its own


class Call:
    """the pool, the CU maps and TWO sets of destination planes in device memory: one for the multi-picture entry, one for the single
    entry called per picture with the table gathered from the pool"""

    def __init__(self, A, pics, pool):
        from kvazaar_amd import _lib as B
        self.A, self.B, self.L, self.pics = A, B, B.load(), pics
        size_of = {}
        for p in pics:
            for r in p["refs"]:
                size_of.setdefault(r, (p["width"], p["height"]))
        self.pool = [None if q is GARBAGE else [A._Staged(v) if v is not None else None for v in q] for q in pool]
        self.n_pool = len(pool)
        self.table = (B.RefPicture * max(self.n_pool, 1))()
        for r, st in enumerate(self.pool):
            if st is None:
                self.table[r] = B.RefPicture(None, None, None, 3, 1, 24, -8)
            else:
                w, h = size_of.get(r, (st[0].w, st[0].h))
                self.table[r] = B.RefPicture(st[0].ptr, st[1].ptr if st[1] else None, st[2].ptr if st[2] else None, st[0].stride,
                                             st[1].stride if st[1] else 0, w, h)
        self.cus = [A.DeviceBuffer.from_numpy(p["cus"].view(np.uint8)) for p in pics]
        self.multi = [[A._Staged(v) if v is not None else None for v in p["dest"]] for p in pics]
        self.single = [[A._Staged(v) if v is not None else None for v in p["dest"]] for p in pics]
        self.records = (B.ReconPicture * max(len(pics), 1))(*[self.record(i, self.multi[i]) for i in range(len(pics))])

    def record(self, i, d):
        p, r = self.pics[i], self.B.ReconPicture()
        r.pred_y, r.pred_u, r.pred_v = d[0].ptr, d[1].ptr if d[1] else None, d[2].ptr if d[2] else None
        r.stride_y, r.stride_c, r.width, r.height, r.cus = d[0].stride, d[1].stride if d[1] else 0, p["width"], p["height"], self.cus[i].ptr
        r.refs[:len(p["refs"])] = p["refs"]
        r.params.chroma, r.params.n_refs = p["chroma"], len(p["refs"])
        C.memmove(r.params.ref_LX, p["ref_LX"].ctypes.data, 32)
        return r

    def run(self, stream=None, records=None, n=None, table=None, n_pool=None):
        """the raw return value of the one call"""
        return self.L.kvz_hip_inter_recon_frames(self.records if records is None else records, len(self.pics) if n is None else n,
                                                 self.table if table is None else table, self.n_pool if n_pool is None else n_pool, stream)

    def run_singles(self, stream=None):
        """kvz_hip_inter_recon_frame per picture: refs[k] = pool[pictures[i].refs[k]]"""
        for i, p in enumerate(self.pics):
            r = self.record(i, self.single[i])
            tab = (self.B.RefPicture * len(p["refs"]))(*[self.table[k] for k in p["refs"]])
            check(self.L.kvz_hip_inter_recon_frame(r.pred_y, r.stride_y, r.pred_u, r.pred_v, r.stride_c, r.width, r.height, r.cus, tab,
                                                   C.byref(r.params), stream), "inter_recon_frame of picture %d" % i)

    def sync(self, stream=None):
        check(self.L.kvz_hip_stream_sync(stream), "sync")

    def results(self, which="multi"):
        """per picture the WHOLE buffers of the three planes"""
        return [tuple(v.download() if v else None for v in d) for d in getattr(self, which)]

    def upload(self, st, a, stream=None):
        a = np.ascontiguousarray(a)
        assert a.shape == st.shape
        check(self.L.kvz_hip_memcpy_h2d(st.buf.ptr, a.ctypes.data, a.nbytes, stream), "h2d")
        self.keep = getattr(self, "keep", []) + [a]

    def poison_again(self, stream=None):
        for which in (self.multi, self.single):
            for d, p in zip(which, self.pics):
                for st, v in zip(d, p["dest"]):
                    if st is not None:
                        self.upload(st, v.buf if isinstance(v, self.A.PlaneView) else v, stream)


def assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for k, n in enumerate("yuv"):
            assert (g[k] is None) == (w[k] is None)
            if g[k] is not None:
                np.testing.assert_array_equal(g[k], w[k], err_msg="%s: picture %d plane %s" % (what, i, n))


def assert_rule(A, pics, pool, what):
    """the one call against the single entry per picture; something was predicted and something left alone in every picture"""
    c = Call(A, pics, pool)
    check(c.run(), "inter_recon_frames (%s)" % what)
    c.sync()
    c.run_singles()
    c.sync()
    got = c.results()
    assert_same(got, c.results("single"), what)
    for i, g in enumerate(got):
        assert (g[0] != POISON).any() and (g[0] == POISON).any(), "%s: picture %d" % (what, i)
    return c, got


# ---------------------------------------------------------------- 1. the three fixture pictures in one call
def test_fixture_pictures_in_one_call(api):
    """200x136 P with 2 references first -- 13 x 9 = 117 tiles, no multiple of four, the last tile column 8 wide and the last tile row 8
    high, so the next picture starts on a rounded workgroup -- then 128x128 B with 4 references and 96x72 4:0:0 with 2: a pool of 8
    pictures of three sizes"""
    z = np.load(GOLDEN, allow_pickle=False)
    pics, pool, wants = [], [], []
    assert [p[:3] for p in IC.FIXTURE_PICTURES] == [("ragged", 200, 136), ("b4", 128, 128), ("mono", 96, 72)]
    for (name, w, h, n_refs, slice_b, chroma, seed) in IC.FIXTURE_PICTURES:
        refs, cus, ref_LX, pus, want = IC.load_fixture_case(z, name, n_refs, chroma)
        pics.append(picture(w, h, range(len(pool), len(pool) + n_refs), cus, ref_LX, chroma))
        pool += refs
        wants.append(want)
    assert len(pool) == 8
    c, got = assert_rule(api, pics, pool, "fixture")
    assert_same(got, wants, "fixture vs tests/golden/inter_recon.npz")


# ---------------------------------------------------------------- 2. a shared pool
W2, H2 = 136, 72
# slots 0, 1, 3, 5: pictures with chroma; 4: luma only, named by the 4:0:0 record alone; 2: garbage, named by nobody
SHARED = (("P", 1201, (0, 1, 3), False, 1), ("B", 1202, (5, 3, 1, 0), True, 1), ("P mono", 1204, (4, 0, 5), False, 0), ("B", 1203, (1, 5, 0, 3), True, 1))


def shared_pool_case():
    planes = IC.random_planes(W2, H2, 1200, 5)
    pool = [planes[0], planes[1], GARBAGE, planes[2], (planes[3][0], None, None), planes[4]]
    pics = [random_picture(W2, H2, seed, refs, slice_b, chroma, bad_share=0.08) for (_, seed, refs, slice_b, chroma) in SHARED]
    return pics, pool


def map_kinds(p):
    """what the PUs of a picture's map cover, from the host-side walk"""
    w, h, n_refs = p["width"], p["height"], len(p["refs"])
    kinds, slots = set(), set()
    for pu in IC.walk_pus(p["cus"], p["ref_LX"], w, h):
        if not IC.pu_valid(pu, w, h, n_refs):
            kinds.add("skipped")
            continue
        d = int(pu["mv_dir"])
        if d == 3:
            kinds.add("bi")
        for lst in range(2):
            if not d & (1 << lst):
                continue
            slots.add(int(pu["ref"][lst]))
            mvx, mvy = int(pu["mv"][lst][0]), int(pu["mv"][lst][1])
            if (mvx & 3) or (mvy & 3):
                kinds.add("fractional")
            if (mvx & 7) == 4 and (mvy & 7) in (0, 4) or (mvy & 7) == 4 and (mvx & 7) == 0:
                kinds.add("luma integer, chroma fractional")
            x0, y0 = int(pu["x"]) + (mvx >> 2) - 3, int(pu["y"]) + (mvy >> 2) - 3
            if x0 < 0 or y0 < 0 or x0 + int(pu["width"]) + 7 > w or y0 + int(pu["height"]) + 7 > h:
                kinds.add("window leaves the picture")
    return kinds, slots


def assert_maps_cover_every_kind_of_pu(pics):
    """no GPU work: the maps of the shared-pool case hold every kind of PU the kernel tells apart, and every slot of every table is used.
    A P picture has no bi-predicted PU by definition (mv_dir is 1 throughout): the B pictures hold them.  A seed that fails here is a bug
    of this test."""
    for (name, seed, refs, slice_b, chroma), p in zip(SHARED, pics):
        kinds, slots = map_kinds(p)
        want = {"fractional", "luma integer, chroma fractional", "window leaves the picture", "skipped"} | ({"bi"} if slice_b else set())
        assert kinds == want, (name, seed, want - kinds)
        assert slots == set(range(len(refs))), (name, seed, slots)


def test_shared_pool_in_a_different_order_per_picture(api):
    """four 136x72 pictures, two P and two B, over five pool pictures and a garbage slot: every picture names three or four of them, each
    in another order; one pool picture has no chroma planes and serves the 4:0:0 record"""
    pics, pool = shared_pool_case()
    assert_maps_cover_every_kind_of_pu(pics)                               # on the CPU, before anything runs
    c, got = assert_rule(api, pics, pool, "shared pool")
    # and the reference's own functions say the same (one P, one B picture: the CPU composition is the slow part)
    planes = [None if q is GARBAGE else q for q in pool]
    for i in (0, 1):
        p = pics[i]
        refs = [planes[r] for r in p["refs"]]
        want = IC.compose(refs, IC.walk_pus(p["cus"], p["ref_LX"], W2, H2), (H2, W2), p["chroma"], poisoned(W2, H2, p["chroma"]))
        assert_same([got[i]], [want], "shared pool vs reference, picture %d" % i)


# ---------------------------------------------------------------- 3. one picture, and sixteen
def test_one_picture(api):
    pool = IC.random_planes(64, 64, 1300, 2)
    assert_rule(api, [random_picture(64, 64, 1302, (1, 0), True)], pool, "one")


SIZES16 = ((64, 64), (72, 40), (96, 72), (40, 136))


def sixteen_case(n=16):
    pics, pool = [], []
    for i in range(n):
        w, h = SIZES16[i % 4]
        pics.append(random_picture(w, h, 1321 + i, (3 * i + 2, 3 * i, 3 * i + 1), i % 2 == 1, 0 if i % 5 == 4 else 1))
        pool += IC.random_planes(w, h, 1340 + i, 3)
    return pics, pool


def test_sixteen_pictures_use_all_48_pool_slots(api):
    pics, pool = sixteen_case()
    assert len(pics) == 16 and len(pool) == 48
    assert_rule(api, pics, pool, "sixteen")


# ---------------------------------------------------------------- 4. padded, offset and unequal strides
def embed(A, plane, stride, left, top, fill, below=3):
    """the plane inside a larger buffer full of `fill`"""
    h, w = plane.shape
    buf = np.full((top + h + below, stride), fill, np.uint8)
    buf[top:top + h, left:left + w] = plane
    return A.PlaneView(buf, w, h, left, top)


def test_padded_offset_and_unequal_strides(api):
    A = api
    w, h = 136, 72
    planes = IC.random_planes(w, h, 1400, 3)
    # every pool picture its own strides and offsets
    pool = [tuple(embed(A, v, v.shape[1] + pad + 4 * (k > 0), 1 + i + k, i, 0xA5) for k, v in enumerate(q)) for i, (q, pad) in enumerate(zip(planes, (5, 24, 11)))]
    assert len({q[0].stride for q in pool}) == 3 and len({q[1].stride for q in pool}) == 3
    pics = []
    for i, (refs, slice_b, chroma) in enumerate((((0, 1, 2), True, 1), ((2, 0), False, 1), ((1, 2), True, 0))):
        dest = tuple(embed(A, v, v.shape[1] + (9, 30, 30)[k] + i, 3 + k, 2 - (k > 0), POISON) if v is not None else None
                     for k, v in enumerate(poisoned(w, h, chroma)))
        assert dest[1] is None or dest[0].stride != 2 * dest[1].stride
        pics.append(random_picture(w, h, 1410 + i, refs, slice_b, chroma, dest))
    c, got = assert_rule(A, pics, pool, "strides")
    for p, g in zip(pics, got):                                            # nothing but the plane inside its buffer was written
        for view, buf in zip(p["dest"], g):
            if view is not None:
                outside = np.ones(buf.shape, dtype=bool)
                view.crop(outside)[:] = False
                assert (buf[outside] == POISON).all()
    # the compact layout gives the same planes
    flat = [picture(w, h, p["refs"], p["cus"], p["ref_LX"], p["chroma"]) for p in pics]
    c2 = Call(A, flat, planes)
    check(c2.run(), "compact")
    c2.sync()
    assert_same([tuple(v.crop(b) if v is not None else None for v, b in zip(p["dest"], g)) for p, g in zip(pics, got)], c2.results(), "padded vs compact")


# ---------------------------------------------------------------- 5. a change in one picture's map
def test_a_change_in_one_picture_leaves_the_others_bit_identical(api):
    pics, pool = sixteen_case(5)
    pool = pool[:15]
    c, before = assert_rule(api, pics, pool, "before")
    other = list(pics)
    other[2] = random_picture(pics[2]["width"], pics[2]["height"], 1500, pics[2]["refs"], True, pics[2]["chroma"])
    c2, after = assert_rule(api, other, pool, "after")                      # picture 2 changes as the single entry says
    for i in range(5):
        if i != 2:
            assert_same([after[i]], [before[i]], "picture %d beside the changed one" % i)
    assert (after[2][0] != before[2][0]).any()


# ---------------------------------------------------------------- 6. one stream, and a graph
def test_four_calls_on_one_stream_and_replayed_from_a_graph_after_the_contents_changed(api):
    A = api
    pics, pool = sixteen_case(8)
    calls = [Call(A, pics[2 * j:2 * j + 2], pool) for j in range(4)]
    L = calls[0].L
    s = L.kvz_hip_stream_create()
    graph = C.c_void_p()
    try:
        for c in calls:                                                    # four asynchronous calls, nothing between them
            check(c.run(s), "inter_recon_frames")
        for c in calls:
            c.run_singles(s)
        check(L.kvz_hip_stream_sync(s), "sync")
        for j, c in enumerate(calls):
            assert_same(c.results(), c.results("single"), "call %d on the stream" % j)
        # one call of four pictures captured, replayed after the CU maps and the pool planes were replaced
        c = Call(A, pics[:4], pool)
        check(L.kvz_hip_graph_begin(s), "graph_begin")
        check(c.run(s), "inter_recon_frames (captured)")
        check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        for round_ in range(2):
            new_pool = [tuple(np.roll(v, 5 + round_, axis=1) ^ np.uint8(0x3C) for v in q) for q in pool]
            for st, q in zip(c.pool, new_pool):
                for v, plane in zip(st, q):
                    c.upload(v, plane, s)
            for i, p in enumerate(c.pics):
                cus, _ = IC.random_cu_map(p["width"], p["height"], 1600 + 10 * round_ + i, len(p["refs"]), i % 2 == 1)
                cus = np.ascontiguousarray(cus)
                check(L.kvz_hip_memcpy_h2d(c.cus[i].ptr, cus.ctypes.data, cus.nbytes, s), "h2d")
                p["cus"] = cus
            c.poison_again(s)
            check(L.kvz_hip_stream_sync(s), "sync")
            check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            check(L.kvz_hip_stream_sync(s), "sync")
            fresh = Call(A, c.pics, new_pool)                              # fresh single-entry calls on the new contents
            fresh.run_singles()
            fresh.sync()
            got = c.results()
            assert_same(got, fresh.results("single"), "replay %d" % round_)
            assert all((g[0] != POISON).any() for g in got)
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


# ---------------------------------------------------------------- 7. refusals
def test_refusals_write_nothing_and_name_the_record(api):
    A = api
    from kvazaar_amd import _lib as B
    # picture 0: 64x64 over slots 0, 1; picture 1: 64x64 over slots 2, 3; picture 2: 72x40 over slot 4, with 2 of 16 table entries in use
    pool = IC.random_planes(64, 64, 1700, 4) + IC.random_planes(72, 40, 1701, 1)
    pics = [random_picture(64, 64, 1710, (0, 1), True), random_picture(64, 64, 1711, (2, 3), True), random_picture(72, 40, 1712, (4, 4), False)]
    c = Call(A, pics, pool)
    L, n = c.L, len(pics)

    def refused(i, what, rec=None, tab=None, **kw):
        recs, table = (B.ReconPicture * n)(*c.records), (B.RefPicture * c.n_pool)(*c.table)
        if rec:
            rec(recs[i])
        if tab:
            tab(table)
        rc = c.run(records=recs, table=table, **kw)
        c.sync()
        assert rc == INVALID, what
        err = L.kvz_hip_last_error()
        assert b"kvz_hip_inter_recon_frames" in err and (b"picture %d" % i) in err, (what, err)
        for g in c.results():
            assert all(v is None or (v == POISON).all() for v in g), what + ": something was written"

    def set_(**fields):
        def f(r):
            for k, v in fields.items():
                setattr(r, k, v)
        return f

    def set_ref(k, v):
        def f(r):
            r.refs[k] = v
        return f

    def set_n_refs(v):
        def f(r):
            r.params.n_refs = v
        return f

    refused(2, "refs[k] >= n_pool", rec=set_ref(1, 5))
    refused(1, "refs[k] >= n_pool, at 255", rec=set_ref(0, 255))
    refused(1, "a named pool picture of another size", tab=lambda t: setattr(t[3], "width", 72))
    refused(0, "a named pool picture of another height", tab=lambda t: setattr(t[1], "height", 56))
    refused(1, "a named pool picture without u", tab=lambda t: setattr(t[2], "u", None))
    refused(0, "a named pool picture without v", tab=lambda t: setattr(t[0], "v", None))
    refused(2, "a named pool picture without y", tab=lambda t: setattr(t[4], "y", None))
    refused(1, "n_refs 0", rec=set_n_refs(0))
    refused(2, "n_refs 17", rec=set_n_refs(17))
    refused(0, "a width that is no multiple of 8", rec=set_(width=60))
    refused(2, "a height that is no multiple of 8", rec=set_(height=36))
    refused(1, "stride_y below the width", rec=set_(stride_y=56))
    refused(0, "stride_c below half the width", rec=set_(stride_c=24))
    refused(2, "a misaligned cus", rec=set_(cus=c.cus[2].ptr + 2))
    refused(1, "cus NULL", rec=set_(cus=None))
    refused(0, "pred_y NULL", rec=set_(pred_y=None))
    refused(1, "pred_u NULL under 4:2:0", rec=set_(pred_u=None))
    refused(2, "pred_y equal to another record's", rec=set_(pred_y=c.records[0].pred_y))
    refused(1, "pred_y equal to a named pool y", rec=set_(pred_y=c.table[4].y))
    refused(0, "pred_v equal to a named pool v", rec=set_(pred_v=c.table[3].v))
    # what is accepted: the same out-of-range index behind n_refs, a garbage slot that nobody names, a named picture without chroma under 4:0:0
    recs = (B.ReconPicture * n)(*c.records)
    for i in range(n):
        for k in range(2, 16):
            recs[i].refs[k] = 255
    table = (B.RefPicture * 6)(*(list(c.table) + [B.RefPicture(None, None, None, 0, 0, 60, 7)]))
    check(c.run(records=recs, table=table, n_pool=6), "accepted")
    c.sync()
    c.run_singles()
    c.sync()
    assert_same(c.results(), c.results("single"), "accepted")
    assert L.kvz_hip_abi_version() == 4


def test_a_49th_reference_and_a_17th_picture_are_refused(api):
    from kvazaar_amd import _lib as B
    c = Call(api, [random_picture(64, 64, 1720, (0,))], IC.random_planes(64, 64, 1721, 1))
    table = (B.RefPicture * 49)(*([c.table[0]] * 49))
    recs = (B.ReconPicture * 17)(*([c.records[0]] * 17))
    for rc in (c.run(table=table, n_pool=49), c.run(n_pool=0), c.run(records=recs, n=17), c.run(n=-1), c.run(table=C.POINTER(B.RefPicture)()),
               c.run(records=C.POINTER(B.ReconPicture)())):
        assert rc == INVALID and b"kvz_hip_inter_recon_frames" in c.L.kvz_hip_last_error()
    assert c.run(records=C.POINTER(B.ReconPicture)(), n=0, table=C.POINTER(B.RefPicture)(), n_pool=0) == 0
    c.sync()
    assert all((v == POISON).all() for v in c.results()[0])


# ---------------------------------------------------------------- 8. the numpy convenience
def test_numpy_convenience_equals_the_ctypes_path(api):
    pics, pool = shared_pool_case()
    c, got = assert_rule(api, pics, pool, "ctypes path")
    conv = api.inter_recon_frames([dict(p, dest=poisoned(W2, H2, p["chroma"])) for p in pics], [None if q is GARBAGE else q for q in pool])
    assert_same(conv, got, "api.inter_recon_frames")
    # device tensors are used where they lie: pool planes, CU maps and destinations
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    on_dev = api.inter_recon_frames([dict(p, cus=up(p["cus"].view(np.uint8)), dest=tuple(up(v) for v in poisoned(W2, H2, p["chroma"]))) for p in pics],
                                    [None if q is GARBAGE else tuple(up(v) for v in q) for q in pool])
    assert all(v is None or v.is_cuda for d in on_dev for v in d)
    assert_same([tuple(None if v is None else v.cpu().numpy() for v in d) for d in on_dev], got, "api.inter_recon_frames on device tensors")
    # default destinations: zeros outside the inter PUs
    zero = api.inter_recon_frames([{k: v for k, v in p.items() if k != "dest"} for p in pics[:2]], [None if q is GARBAGE else q for q in pool])
    for z, g in zip(zero, got):
        for a, b in zip(z, g):
            if b is not None:
                m = b != POISON
                assert m.any() and (a[m] == b[m]).all() and ((a[~m] == 0) | (a[~m] == POISON)).all()


# ---------------------------------------------------------------- 9. the chain
def test_chain_prediction_residual_deblocking_of_two_pictures(api):
    """two 128x128 P pictures that share one reference through kvz_hip_inter_recon_frames -> kvz_hip_inter_residual_frames ->
    kvz_hip_deblock_frames: the bytes (rec, coeff, cus) of the three single-picture entries run per picture"""
    import test_gpu_chain_multi as CM
    import test_gpu_inter_residual as TR
    import test_gpu_intra_recon as TX
    from kvazaar_amd import _lib as B
    A, w, h, qp = api, 128, 128, 30
    L = B.load()
    refs = IC.random_planes(w, h, 1900, 1)
    cases = []
    for i in range(2):
        cus, ref_LX = RC.make_map(w, h, 1901 + i, n_refs=1, slice_b=False, intra_share=0.1, blank_share=0.0, bad_share=0.0, edge_cu=False)
        dest = tuple(np.full((h >> (1 if k else 0), w >> (1 if k else 0)), RC.POISON_PIXEL, np.uint8) for k in range(3))
        src = RC.make_source(refs[0], cus, 1910 + i, 1)
        cases.append((cus, ref_LX, dest, src))
    s = L.kvz_hip_stream_create()
    try:
        # the single-picture entries, per picture
        singles = [TR.Chain(A, refs, cus, ref_LX, dest, src, qp, False) for (cus, ref_LX, dest, src) in cases]
        for ch in singles:
            ch.launch(s)
        check(L.kvz_hip_stream_sync(s), "sync")
        want = [ch.st.result() for ch in singles]
        # the three multi-picture entries on stagings of their own; the record of the residual stage is the existing chain test's
        pool = B.RefPicture.from_buffer_copy(singles[0].recon.table[0].tobytes())
        sts, recon, resid, filt = [], (B.ReconPicture * 2)(), (B.ChainPicture * 2)(), (B.FilterPicture * 2)()
        for i, (cus, ref_LX, dest, src) in enumerate(cases):
            init = (tuple(np.zeros_like(v) for v in RC.initial_outputs(w, h)[0]), np.zeros(cus.shape, np.uint8), np.zeros(cus.shape, RC.COST))
            st = TX.Staged(A, src, dest, cus, np.zeros(cus.shape + (2,), np.uint8), qp, 1, 0, 0, init=init)
            sts.append(st)
            r = recon[i]
            r.pred_y, r.pred_u, r.pred_v, r.stride_y, r.stride_c = st.ptr("rec", 0), st.ptr("rec", 1), st.ptr("rec", 2), w, w // 2
            r.width, r.height, r.cus = w, h, st.ptr("cus")
            r.refs[0], r.params.chroma, r.params.n_refs = 0, 1, 1
            C.memmove(r.params.ref_LX, np.ascontiguousarray(ref_LX, dtype=np.uint8).ctypes.data, 32)
            resid[i] = CM.record(st, False)
            f = filt[i]
            f.width, f.height, f.chroma = w, h, 1
            f.rec_y, f.rec_u, f.rec_v, f.stride_y, f.stride_c, f.cus = st.ptr("rec", 0), st.ptr("rec", 1), st.ptr("rec", 2), w, w // 2, st.ptr("cus")
            dprm = deblock_params(qp=qp, slice_is_b=0, chroma=1)
            dprm["ref_LX"] = ref_LX
            f.deblock = B.DeblockParams.from_buffer_copy(np.ascontiguousarray(dprm).tobytes())
        check(L.kvz_hip_inter_recon_frames(recon, 2, C.byref(pool), 1, s), "inter_recon_frames")        # three calls, nothing between them
        check(L.kvz_hip_inter_residual_frames(resid, 2, s), "inter_residual_frames")
        check(L.kvz_hip_deblock_frames(filt, 2, s), "deblock_frames")
        check(L.kvz_hip_stream_sync(s), "sync")
        for i, st in enumerate(sts):
            got = st.result()
            for k in range(3):
                np.testing.assert_array_equal(got["rec"][k], want[i]["rec"][k], err_msg="picture %d: rec plane %d after the chain" % (i, k))
                np.testing.assert_array_equal(got["coeff"][k], want[i]["coeff"][k], err_msg="picture %d: coeff %d" % (i, k))
            np.testing.assert_array_equal(got["cus"].view(np.uint8), want[i]["cus"].view(np.uint8), err_msg="picture %d: cus" % i)
            assert (got["rec"][0] != RC.POISON_PIXEL).any() and any((c != 0).any() for c in got["coeff"])
    finally:
        L.kvz_hip_stream_destroy(s)

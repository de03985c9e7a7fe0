"""GPU: the multi-picture entries with RDOQ -- kvz_hip_inter_residual_frames_rdoq and kvz_hip_intra_recon_frames_rdoq -- against
tests/golden/rdoq_chain.npz (every TU from the compiled reference's own kvz_quantize_residual under cfg.rdoq_enable) and against the
single-picture _rdoq entries on a second staging of the same inputs.  The pictures are the four of the fixture: `ragged` 200 x 136 (also
tiled), `mono` 96 x 72 4:0:0, `coarse` 256 x 128, `deep` 128 x 64: rows, tile columns, wavefronts and slots of one picture run out while
another's go on.  One staging per picture, every array between guard bands; every comparison is exact.  Every test runs under a time
limit of its own that ends the process, and after a call that reports a runtime error no further test starts anything on the device."""
import ctypes as C
import faulthandler
import os
import sys

import numpy as np
import pytest

import inter_residual_cases as RC
import lcu_qp_cases as QC
import rdoq_chain_cases as K
import test_gpu_chain_multi as MC
import test_gpu_rdoq_chain as T
import test_gpu_scaling_list as SLT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PICS = {p[0]: p for p in K.PICTURES}
INVALID = SLT.INVALID
check = SLT.check
TEST_LIMIT_S = 60
FAULTS = []
INTER, INTRA = "kvz_hip_inter_residual_frames_rdoq", "kvz_hip_intra_recon_frames_rdoq"


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


_LOADED = {}


def npz(name):
    if name not in _LOADED:
        _LOADED[name] = np.load(os.path.join(HERE, "golden", name), allow_pickle=False)
    return _LOADED[name]


def tables_of(lists):
    """0: flat, 1: default -> (the RDOQ tables (quant, err_scale), the scaling tables (quant, dequant) or None); loaded once, never changed"""
    r, s = npz("rdoq.npz"), npz("scaling_list.npz")
    return ((r["quant"][lists], r["err_scale"][lists]), (s["default_quant"], s["default_dequant"]) if lists else None)


def guarded(what, f, *args):
    """a call that may meet the device: a runtime error ends the session's device work"""
    try:
        return f(*args)
    except Exception as e:
        if not isinstance(e, AssertionError) or "runtime" in str(e) or "HIP" in str(e):
            FAULTS.append(what)
        raise


class Staged(T.Staged):
    """the staging of test_gpu_rdoq_chain with the settings of the fixture as arguments: which scaling tables, which RDOQ tables, the
    picture's own sets and states, its lcu_ctx or None, rdoq_skip"""

    def __init__(self, A, case, lists, sets, states, lcu_ctx, skip):
        from kvazaar_amd import _lib
        rq_tables, scaling = tables_of(lists)
        SLT.Staged.__init__(self, A, case, scaling)
        self.host["sets"], self.host["states"] = [np.ascontiguousarray(sets)], [np.ascontiguousarray(states)]
        self.host["rq_quant"], self.host["rq_err"] = [np.ascontiguousarray(rq_tables[0], np.int32)], [np.ascontiguousarray(rq_tables[1], np.float64)]
        if lcu_ctx is not None:
            self.host["lcu_ctx"] = [np.ascontiguousarray(lcu_ctx, np.uint16)]
        for k in ("sets", "states", "rq_quant", "rq_err", "lcu_ctx"):
            if k in self.host:
                self.dev[k] = [self._up(self.host[k][0])]
        self.rq = _lib.RdoqSource(self.ptr("sets"), self.ptr("states"), self.ptr("lcu_ctx") if lcu_ctx is not None else None,
                                  _lib.RdoqTables(self.ptr("rq_quant"), self.ptr("rq_err")), len(sets), skip)


class Item:
    """one picture of a call: a picture of the fixture with the fixture's settings (K.SETTINGS) unless said otherwise.  grid: (col_bd,
    row_bd) or None; rotate: the picture's sets and states are the fixture's rotated by that many places; stages: which entries it goes
    through; want: the fixture's tags after the inter and after the intra stage, or None"""

    def __init__(self, name, grid=None, skip=None, lists=None, ctx=None, per_lcu=True, cbf=True, costs=True, rotate=0, stages=("inter", "intra"), want=None,
                 src=None):
        self.name, self.grid, self.per_lcu, self.cbf, self.costs, self.rotate, self.stages, self.want, self.src = name, grid, per_lcu, cbf, costs, rotate, stages, want, src
        s = K.SETTINGS[name]
        self.skip, self.ctx, self.lists = s[0] if skip is None else skip, s[1] if ctx is None else ctx, s[2] if lists is None else lists
        self.pic = PICS[name]
        self.w, self.h, self.chroma = self.pic[1:4]

    def but(self, **kw):
        d = dict(grid=self.grid, skip=self.skip, lists=self.lists, ctx=self.ctx, per_lcu=self.per_lcu, cbf=self.cbf, costs=self.costs, rotate=self.rotate,
                 stages=self.stages, want=self.want, src=self.src)
        d.update(kw)
        return Item(self.name, **d)

    def case(self):
        case = T.case_dict(self.pic, K.load_inputs(npz("lcu_qp.npz"), self.pic, npz("rdoq_chain.npz")), self.grid)
        case["per_lcu"] = self.per_lcu
        if self.src is not None:
            case["src"] = self.src
        return case

    def source(self, A):
        sets, states = K.records(A)
        lcu_ctx = None
        if self.ctx:
            # the fixture's array, or for a picture whose fixture has none the same rule: by LCU position
            lx, ly = QC.lcu_grid(self.w, self.h)
            lcu_ctx = K.lcu_ctx_of(self.name, self.w, self.h) if K.SETTINGS[self.name][1] else ((np.arange(lx * ly) * 5 + 1) % K.N_SETS).astype(np.uint16)
        return np.roll(sets, self.rotate), np.roll(states, self.rotate), lcu_ctx

    def poison(self):
        return RC.initial_outputs(self.w, self.h, self.chroma)

    def stage(self, A, init=None):
        sets, states, lcu_ctx = self.source(A)
        st = Staged(A, self.case(), self.lists, sets, states, lcu_ctx, self.skip)
        if init is not None:
            for k in range(3 if self.chroma else 1):
                st.upload("coeff", k, init[0][k])
            st.upload("cbf_out", 0, init[1])
            st.upload("costs", 0, init[2])
        return st

    def record(self, st, rdoq=True):
        from kvazaar_amd import _lib as B
        r = B.ChainPictureRdoq()
        r.pic = MC.record(st, self.per_lcu, self.cbf, self.costs)
        if st.grid is not None:
            r.grid = C.cast(st.grid.ctypes.data, C.POINTER(B.TileGrid))
        if st.sl is not None:
            r.tables = st.sl
        if rdoq:
            r.rdoq = C.pointer(st.rq)
        return r

    def single(self, st, stage, stream=None, **over):
        """the single-picture _rdoq entry of that stage with this picture's fields"""
        if not self.cbf:
            over["cbf"] = None
        if not self.costs:
            over["costs"] = None
        if stage == "inter":
            check(st.inter_rdoq(stream, **over), "inter_residual_frame_rdoq")
        else:
            check(st.intra_rdoq(stream, **over), "intra_recon_frame_rdoq")


class Batch:
    """stagings and records of one call of each entry.  The RDOQ tables of a call are those of its first staging: the entries require
    one pair of pointers, and every staging of a call holds the same values"""

    def __init__(self, A, its, init=None, rdoq=True):
        from kvazaar_amd import _lib as B
        self.B, self.items, self.L = B, list(its), B.load()
        self.st = [it.stage(A, init[i] if init else None) for i, it in enumerate(self.items)]
        for st in self.st[1:]:
            np.testing.assert_array_equal(st.host["rq_quant"][0], self.st[0].host["rq_quant"][0])
            st.rq.tables = self.st[0].rq.tables
        self.records = (B.ChainPictureRdoq * max(len(self.items), 1))(*[it.record(st, rdoq) for it, st in zip(self.items, self.st)])

    def subset(self, stage):
        keep = [i for i, it in enumerate(self.items) if stage in it.stages]
        return (self.B.ChainPictureRdoq * max(len(keep), 1))(*[self.records[i] for i in keep]), len(keep)

    def run(self, stage, stream=None):
        recs, n = self.subset(stage)
        entry = self.L.kvz_hip_inter_residual_frames_rdoq if stage == "inter" else self.L.kvz_hip_intra_recon_frames_rdoq
        guarded(stage, lambda: check(entry(recs, n, stream), INTER if stage == "inter" else INTRA))

    def sync(self, stream=None):
        guarded("sync", lambda: check(self.L.kvz_hip_stream_sync(stream), "sync"))

    def results(self):
        return [st.result() for st in self.st]


def equal(got, want, what, chroma):
    RC.assert_outputs_equal(got, want, what, chroma)


def assert_rule(A, its, what):
    """the multi entries on one staging against the single _rdoq entries on a second one, both over poisoned outputs, stage by stage"""
    init = [it.poison() for it in its]
    b = Batch(A, its, init)
    singles = [it.stage(A, init[i]) for i, it in enumerate(its)]
    for stage in ("inter", "intra"):
        b.run(stage)
        b.sync()
        for it, st, single in zip(its, b.st, singles):
            if stage not in it.stages:
                continue
            guarded("the single entry", it.single, single, stage)
            guarded("sync", single.sync)
            equal(st.result(), single.result(), "%s, %s: %s" % (what, stage, it.name), it.chroma)
    for i, (it, got) in enumerate(zip(its, b.results())):
        if not it.cbf:
            assert (got["cbf_out"] == init[i][1]).all(), "cbf_out was written though NULL was passed"
        if not it.costs:
            np.testing.assert_array_equal(got["costs"].view(np.uint32), init[i][2].view(np.uint32), err_msg="costs were written though NULL was passed")
        assert any((c != RC.POISON_COEFF).any() for c in got["coeff"] if c is not None), "nothing was coded"
    return b


def want_of(tag, chroma):
    return K.load_want(npz("rdoq_chain.npz"), tag, chroma)


def run_fixture(A, its, what):
    """both entries over zeroed outputs; each picture against its fixture after each stage"""
    b = Batch(A, its)
    for k, stage in enumerate(("inter", "intra")):
        b.run(stage)
        b.sync()
        for it, got in zip(its, b.results()):
            if it.want is not None and it.want[k] is not None:
                equal(got, want_of(it.want[k], it.chroma), "%s, %s: %s" % (what, stage, it.want[k]), it.chroma)
    return b


RAGGED = Item("ragged", want=("ragged_mid", "ragged_full"))
TILED = Item("ragged", grid=K.TILE_GRID["ragged"], want=("ragged_mid", "ragged_tiled"))
DEEP = Item("deep", want=("deep_mid", "deep_full"))
COARSE = Item("coarse", want=("coarse_mid", "coarse_full"))
MONO = Item("mono", want=("mono_mid", "mono_full"))


# ---------------------------------------------------------------- 1. the fixture through the multi entries
def test_fixture_flat_lists_tiled_beside_untiled(api):
    b = run_fixture(api, [RAGGED, TILED, DEEP], "flat")
    assert [bool(b.records[i].grid) for i in range(3)] == [False, True, False]
    assert (want_of("ragged_tiled", 1)["rec"][0] != want_of("ragged_full", 1)["rec"][0]).any()


def test_fixture_default_lists(api):
    # `coarse` twice: the second with a context set per picture of its own is covered below; here the fixture's settings, and a second
    # record of the same picture so that the call holds more than one
    b = run_fixture(api, [COARSE, COARSE], "default lists")
    assert b.records[0].tables.quant and b.records[0].tables.quant != b.records[1].tables.quant


def test_fixture_mono_with_rdoq_skip(api):
    b = run_fixture(api, [MONO], "skip")
    assert b.records[0].rdoq.contents.rdoq_skip == 1 and not b.records[0].pic.params.chroma


# ---------------------------------------------------------------- 2. the rule
@pytest.mark.parametrize("lists", [0, 1])
@pytest.mark.parametrize("skip", [0, 1])
def test_equals_the_single_picture_entries(api, lists, skip):
    """mixed sizes and chroma formats, tiled beside untiled, with and without lcu_qp / cbf_out / costs / lcu_ctx"""
    its = [MONO.but(ctx=True, cbf=True, costs=True), RAGGED.but(cbf=True, costs=False, ctx=False), TILED.but(per_lcu=False, cbf=False, costs=True),
           DEEP.but(cbf=False, costs=False), COARSE.but(per_lcu=False, cbf=True, costs=False)]
    its = [it.but(lists=lists, skip=skip, want=None) for it in its]
    assert {it.chroma for it in its} == {0, 1} and {it.per_lcu for it in its} == {True, False} and {it.ctx for it in its} == {True, False}
    assert len({(it.w, it.h) for it in its}) == 4
    assert_rule(api, its, "lists %d, skip %d" % (lists, skip))


# ---------------------------------------------------------------- 3. per-picture sources
def test_every_picture_has_its_own_context_sets_and_states(api):
    """the sets and states rotated by the picture's index, with and without lcu_ctx: each picture equals the single entry on its own
    source, and the sources give different outputs -- a kernel that read picture 0's source for everyone would not pass"""
    its = [RAGGED.but(rotate=k, ctx=bool(k & 1), want=None) for k in range(4)]
    b = assert_rule(api, its, "own sources")
    got = b.results()
    for k in range(1, 4):
        assert any((a != c).any() for a, c in zip(got[k]["coeff"], got[0]["coeff"])), "picture %d: the outputs of two sources do not differ" % k
    assert len({(b.records[k].rdoq.contents.ctx_sets, b.records[k].rdoq.contents.states) for k in range(4)}) == 4
    # and n_sets is the picture's own: one set alone, every index beyond it
    one = [RAGGED.but(want=None), DEEP.but(rotate=2, want=None)]
    b = Batch(api, one, [it.poison() for it in one])
    b.st[1].rq.n_sets = 1
    single = one[1].stage(api, one[1].poison())
    single.rq.n_sets = 1
    for stage in ("inter", "intra"):
        b.run(stage)
        guarded("the single entry", one[1].single, single, stage)
    b.sync()
    equal(b.st[1].result(), single.result(), "n_sets of the picture's own", 1)


# ---------------------------------------------------------------- 4. sixteen pictures, order, one
def test_sixteen_pictures_order_and_one(api):
    five = [RAGGED, TILED, DEEP, MONO.but(skip=0, want=None), RAGGED.but(rotate=3, want=None)]
    sixteen = (five * 4)[:16]
    b = run_fixture(api, sixteen, "sixteen")
    assert len(b.st) == 16 and len({st.ptr("rec", 0) for st in b.st}) == 16
    fwd, rev = b.results()[:5], run_fixture(api, five[::-1], "reversed").results()[::-1]
    for it, a, c in zip(five, fwd, rev):
        equal(a, c, "order: " + it.name, it.chroma)
    for it in (RAGGED, TILED, DEEP, COARSE, MONO):
        run_fixture(api, [it], "alone")


# ---------------------------------------------------------------- 5. no record carries rdoq
def test_without_rdoq_it_is_the_frames_ts_entries(api):
    its = [TILED.but(want=None), MONO.but(want=None), DEEP.but(per_lcu=False, want=None)]
    new, old = Batch(api, its, rdoq=False), Batch(api, its, rdoq=False)
    B, L = old.B, old.L
    for stage, entry in (("inter", L.kvz_hip_inter_residual_frames_ts), ("intra", L.kvz_hip_intra_recon_frames_ts)):
        new.run(stage)
        recs, n = old.subset(stage)
        ts = (B.ChainPictureTs * n)()
        for i in range(n):
            ts[i].pic, ts[i].grid, ts[i].tables = recs[i].pic, recs[i].grid, recs[i].tables
        guarded("frames_ts", lambda: check(entry(ts, n, None), "the _frames_ts entry"))
    new.sync()
    for it, a, c in zip(its, new.results(), old.results()):
        equal(a, c, "no rdoq: " + it.name, it.chroma)
    # RDOQ is not the plain quantiser on these pictures
    assert any((a != c).any() for a, c in zip(new.results()[0]["coeff"], want_of("ragged_tiled", 1)["coeff"]))
    # and a refusal is that entry's, word for word: it names itself, or for the inter stage, where these records carry no option that it
    # reads, the plain multi-picture entry that it calls in turn
    bad = new.subset("inter")[0]
    bad[1].pic.cus = None
    ts = (B.ChainPictureTs * 3)()
    for i in range(3):
        ts[i].pic, ts[i].grid, ts[i].tables = bad[i].pic, bad[i].grid, bad[i].tables
    for name, said in ((INTER, b"kvz_hip_inter_residual_frames:"), (INTRA, b"kvz_hip_intra_recon_frames_ts:")):
        assert getattr(L, name.replace("_rdoq", "_ts"))(ts, 3, None) == INVALID
        want = L.kvz_hip_last_error()
        assert getattr(L, name)(bad, 3, None) == INVALID and L.kvz_hip_last_error() == want
        assert want.startswith(said) and b"picture 1 (" in want, want


# ---------------------------------------------------------------- 6. refusals
def test_refusals_write_nothing_and_name_the_record(api):
    from kvazaar_amd import _lib as B
    flat, lists = [RAGGED, MONO.but(skip=0), DEEP, TILED], [COARSE, COARSE.but(rotate=1), RAGGED.but(lists=1)]
    bf, bl = Batch(api, flat, [it.poison() for it in flat]), Batch(api, lists, [it.poison() for it in lists])
    L = bf.L
    before = [b.results() for b in (bf, bl)]
    keep = []

    def bad(b, at, **fields):
        n = len(b.items)
        recs = (B.ChainPictureRdoq * n)(*[b.records[i] for i in range(n)])
        src = {}
        for k, v in fields.items():
            if k == "scaling_list":
                recs[at].pic.params.scaling_list = v
            elif k in ("cus", "rec_y", "coeff_y"):
                setattr(recs[at].pic, k, v)
            elif k in ("tables", "grid", "rdoq"):
                setattr(recs[at], k, v)
            else:
                src[k] = v
        if src:
            g = b.records[at].rdoq.contents
            f = dict(ctx_sets=g.ctx_sets, states=g.states, lcu_ctx=g.lcu_ctx, quant=g.tables.quant, err_scale=g.tables.err_scale, n_sets=g.n_sets,
                     rdoq_skip=g.rdoq_skip)
            f.update(src)
            keep.append(B.RdoqSource(f["ctx_sets"], f["states"], f["lcu_ctx"], B.RdoqTables(f["quant"], f["err_scale"]), f["n_sets"], f["rdoq_skip"]))
            recs[at].rdoq = C.pointer(keep[-1])
        return recs, n, at

    some, none = bl.records[0].tables, B.ScalingTables(None, None)
    g0 = bf.records[0].rdoq.contents
    short = api.tile_grid(flat[3].w, flat[3].h, [0, 1, 2], K.TILE_GRID["ragged"][1])         # the last boundary is 2 of 4 LCUs
    short_p = C.cast(short.ctypes.data, C.POINTER(B.TileGrid))
    both = [
        bad(bf, 2, tables=some, scaling_list=1),                 # tables among records without
        bad(bl, 1, tables=none, scaling_list=0),                 # none among records with
        bad(bf, 1, rdoq=None),                                   # a record without rdoq among records with
        bad(bf, 3, rdoq_skip=1),                                 # rdoq_skip other than record 0's
        bad(bf, 2, quant=bl.records[0].rdoq.contents.tables.quant),          # RDOQ tables other than record 0's
        bad(bf, 1, err_scale=bl.records[0].rdoq.contents.tables.err_scale),
        bad(bf, 2, ctx_sets=None), bad(bf, 3, states=None), bad(bl, 1, n_sets=0),
        bad(bf, 1, ctx_sets=g0.ctx_sets + 1), bad(bf, 0, lcu_ctx=g0.lcu_ctx + 1), bad(bf, 2, states=g0.states + 4),
        bad(bf, 1, scaling_list=1), bad(bl, 2, scaling_list=0), bad(bl, 1, tables=B.ScalingTables(some.quant, None)),
        bad(bf, 2, cus=None), bad(bf, 3, rec_y=bf.records[1].pic.rec_y), bad(bl, 2, coeff_y=bl.records[0].pic.coeff_y),
    ]
    intra_only = [bad(bf, 3, grid=short_p)]                      # the inter stage does not read the grid
    for name in (INTER, INTRA):
        entry = getattr(L, name)
        for recs, n, at in both + (intra_only if name == INTRA else []):
            assert entry(recs, n, None) == INVALID, at
            assert b"picture %d (" % at in L.kvz_hip_last_error() and name.encode() in L.kvz_hip_last_error(), (at, L.kvz_hip_last_error())
        assert entry(bf.records, 0, None) == 0 and entry(None, 0, None) == 0
        assert entry(bf.records, 17, None) == INVALID and entry(bf.records, -1, None) == INVALID and entry(None, 3, None) == INVALID
    # the pool of boundaries: 1024 x 512 pictures on the pointers of the first staging, moved apart, the last record without coeff_y so
    # that no such call can launch anything.  9 x 26 + 22 = 256 fit and the call goes on to its last record; 9 x 26 + 19 + 4 = 257 do not
    grids = []

    def fabricated(shapes):
        recs = (B.ChainPictureRdoq * len(shapes))()
        for i, shape in enumerate(shapes):
            r = recs[i]
            C.memmove(C.byref(r), C.byref(bf.records[0]), C.sizeof(r))
            r.pic.src.width, r.pic.src.height = 1024, 512
            r.pic.src.stride_y = r.pic.stride_y = 1024
            r.pic.src.stride_c = r.pic.stride_c = 512
            r.pic.rec_y, r.pic.cus, r.pic.coeff_y = r.pic.rec_y + 64 * i, r.pic.cus + 64 * i, r.pic.coeff_y + 64 * i
            r.grid = None
            if shape:
                g = B.TileGrid()
                g.cols, g.rows = shape
                for j in range(shape[0] + 1):
                    g.col_bd[j] = j * 16 // shape[0]
                for j in range(shape[1] + 1):
                    g.row_bd[j] = j * 8 // shape[1]
                grids.append(g)
                r.grid = C.pointer(g)
        recs[len(shapes) - 1].pic.coeff_y = None
        return recs, len(shapes)

    assert B.CHAIN_TILE_BOUNDS == 256
    recs, n = fabricated([(16, 8)] * 9 + [(12, 8), None, None])
    assert L.kvz_hip_intra_recon_frames_rdoq(recs, n, None) == INVALID and b"picture 11 (" in L.kvz_hip_last_error(), L.kvz_hip_last_error()
    recs, n = fabricated([(16, 8)] * 9 + [(9, 8), (1, 1), None])
    assert L.kvz_hip_intra_recon_frames_rdoq(recs, n, None) == INVALID and b"picture 10 (" in L.kvz_hip_last_error(), L.kvz_hip_last_error()
    assert b"KVZ_HIP_CHAIN_TILE_BOUNDS" in L.kvz_hip_last_error()
    bf.sync()
    for b, was in zip((bf, bl), before):
        for it, got, want in zip(b.items, b.results(), was):
            equal(got, want, it.name + " after refused calls", it.chroma)
            assert any((c == RC.POISON_COEFF).all() for c in got["coeff"] if c is not None)
    assert L.kvz_hip_abi_version() == 4


# ---------------------------------------------------------------- 7. graph
def test_both_calls_replayed_from_a_graph_after_the_contents_changed(api):
    """a tiled picture, a 4:0:0 picture and `deep`, captured on one stream; the replay runs on other sources, context sets and states in
    two of the three pictures and equals the single entries run on those"""
    its = [TILED.but(want=None), MONO.but(skip=0, want=None), DEEP.but(want=None)]
    b = Batch(api, its)
    L, s, graph = b.L, b.L.kvz_hip_stream_create(), C.c_void_p()
    try:
        guarded("graph_begin", lambda: check(L.kvz_hip_graph_begin(s), "graph_begin"))
        b.run("inter", s)
        b.run("intra", s)
        guarded("graph_end", lambda: check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end"))
        assert graph.value
        flipped = tuple(np.ascontiguousarray(p[::-1, ::-1]) for p in its[0].case()["src"])
        changed = [its[0].but(src=flipped, rotate=2), its[1], its[2].but(rotate=4)]
        wants = {}
        for run, now in (("first launch", its), ("replay", changed)):
            want = wants[run] = []
            for it, st in zip(now, b.st):
                single = it.stage(api)
                guarded("the single entries", lambda: (it.single(single, "inter"), it.single(single, "intra"), single.sync()))
                want.append(single.result())
                for kind in ("src", "sets", "states"):
                    for k, a in enumerate(single.host[kind]):
                        st.upload(kind, k, a, s)
                        st.host[kind][k] = np.ascontiguousarray(a)
                for kind in ("rec", "coeff", "cus", "cbf_out", "costs"):
                    for k, a in enumerate(st.host[kind]):
                        st.upload(kind, k, a, s)
            b.sync(s)
            guarded("graph_launch", lambda: check(L.kvz_hip_graph_launch(graph, s), "graph_launch"))
            b.sync(s)
            for it, st, w in zip(now, b.st, want):
                equal(st.result(), w, "%s: %s" % (run, it.name), it.chroma)
        for i in (0, 2):
            assert any((a != c).any() for a, c in zip(wants["replay"][i]["coeff"], wants["first launch"][i]["coeff"])), "the replay ran on other contents"
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


# ---------------------------------------------------------------- 8. numpy conveniences
def test_numpy_conveniences_on_a_tiled_batch(api):
    its = [RAGGED, TILED, DEEP.but(rotate=1, want=None)]

    def rdoq(it):
        sets, states, lcu_ctx = it.source(api)
        return dict(sets=sets, states=states, tables=tables_of(it.lists)[0], lcu_ctx=lcu_ctx, skip=it.skip)

    first = []
    for it in its:
        c, init = it.case(), QC.zero_outputs(it.w, it.h, it.chroma)
        first.append(dict(src=c["src"], pred=c["pred"], cus=c["cus"], qp=c["qp"], chroma=it.chroma, slice_is_intra=c["slice_is_intra"], signhide=c["signhide"],
                          coeff=init[0], cbf_out=init[1], costs=init[2], lcu_qp=c["lcu_qp"], rdoq=rdoq(it)))
    mid = guarded("the conveniences", api.inter_residual_frames_rdoq, first)
    second = []
    for it, d, m in zip(its, first, mid):
        d = dict(d, rec=m["rec"], cus=m["cus"], modes=it.case()["modes"], coeff=m["coeff"], cbf_out=m["cbf_out"], costs=m["costs"])
        del d["pred"]
        if it.grid:
            d["grid"] = it.grid
        second.append(d)
    full = guarded("the conveniences", api.intra_recon_frames_rdoq, second)
    for it, m, f in zip(its[:2], mid, full):
        RC.assert_outputs_equal(m, want_of(it.want[0], it.chroma), it.want[0] + " convenience", it.chroma)
        RC.assert_outputs_equal(f, want_of(it.want[1], it.chroma), it.want[1] + " convenience", it.chroma)
    # the third picture has sources of its own: the single conveniences on the same dicts
    d = dict(first[2])
    one = api.inter_residual_frame(d["src"], d["pred"], d["cus"], d["qp"], d["chroma"], d["slice_is_intra"], d["signhide"], coeff=d["coeff"], cbf_out=d["cbf_out"],
                                   costs=d["costs"], lcu_qp=d["lcu_qp"], rdoq=d["rdoq"])
    RC.assert_outputs_equal(mid[2], one, "deep, rotated sets: convenience", 1)

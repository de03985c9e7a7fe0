"""GPU: the multi-picture entries that take tiles, scaling lists and transform skip -- kvz_hip_inter_residual_frames_ts and
kvz_hip_intra_recon_frames_ts -- against the committed fixtures (tile_chain.npz, scaling_list.npz, trskip.npz, lcu_qp.npz, intra_recon.npz)
and against the single-picture _ts entries on a second staging of the same inputs.  The pictures of one call differ in size (72 x 72 to
256 x 192: rows, tile columns and wavefronts of one picture run out while another's go on), in their tile grid (tiled beside untiled), in
chroma format, QP, sign hiding and slice type, in the tables they point to and in whether they carry lcu_qp, lcu_bit_cost, cbf_out and
costs.  One staging per picture (test_gpu_trskip.Staged): every array between guard bands, tr_skip_out poisoned and at an odd address,
the QP array at an odd address; every comparison is exact.  After a call or a synchronisation that reports a runtime error no further
test starts anything on the device."""
import ctypes as C
import faulthandler
import sys

import numpy as np
import pytest

import inter_residual_cases as RC
import lcu_qp_cases as QC
import scaling_list_cases as SL
import test_gpu_chain_multi as MC
import test_gpu_scaling_list as GS
import test_gpu_tile_chain as TT
import test_gpu_trskip as TS
import tile_chain_cases as TC
import trskip_cases as T

pytestmark = pytest.mark.gpu

INVALID = -2
check = TS.check


@pytest.fixture(autouse=True)
def limits():
    assert not TS.FAULTS, "an earlier test met a device error (%s): nothing more is started" % TS.FAULTS[0]
    faulthandler.dump_traceback_later(TS.TEST_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


class Item:
    """one picture of a call: its case (the dict the stagings of test_gpu_scaling_list / test_gpu_trskip take), the stages it goes
    through, what they leave according to its fixture (or None), its tables (packed pair or None), whether it carries ts and with which
    bit cost (an int, or an array for lcu_bit_cost), the initial contents of its outputs where they are not zeros, and whether cbf_out
    and costs are passed"""

    def __init__(self, name, case, stages, want=None, tables=None, ts=False, bit_cost=None, init=None, cbf=True, costs=True):
        self.name, self.case, self.stages, self.want, self.tables, self.ts, self.init, self.cbf, self.costs = name, case, stages, want, tables, ts, init, cbf, costs
        self.bit_cost = (case["bit_cost"] if bit_cost is None else bit_cost) if ts else 0
        self.chroma = case["chroma"]

    def but(self, **kw):
        new = Item(self.name, self.case, self.stages, self.want, self.tables, self.ts, self.bit_cost if self.ts else None, self.init, self.cbf, self.costs)
        for k, v in kw.items():
            setattr(new, k, v)
        if "case" in kw:
            new.chroma = new.case["chroma"]
        return new

    def stage(self, A, init=None):
        st = TS.Staged(A, self.case, self.tables, bit_cost=self.bit_cost)
        init = init or self.init
        if init is not None:
            for k in range(3 if self.chroma else 1):
                st.upload("coeff", k, init[0][k])
            st.upload("cbf_out", 0, init[1])
            st.upload("costs", 0, init[2])
        return st

    def poison(self):
        return RC.initial_outputs(self.case["width"], self.case["height"], self.chroma)

    def record(self, st):
        from kvazaar_amd import _lib as B
        r = B.ChainPictureTs()
        r.pic = MC.record(st, self.case["per_lcu"], self.cbf, self.costs)
        if st.grid is not None:
            r.grid = C.cast(st.grid.ctypes.data, C.POINTER(B.TileGrid))
        if st.sl is not None:
            r.tables = st.sl
        if self.ts:
            r.ts, r.tr_skip_out = C.pointer(st.ts), st.ptr("tr_skip") + st.odd
        return r

    def single(self, st, stream=None):
        """the single-picture _ts entries with this picture's fields"""
        over = {}
        if not self.ts:
            over.update(ts=None, skip=None)
        if not self.cbf:
            over["cbf"] = None
        if not self.costs:
            over["costs"] = None
        if "inter" in self.stages:
            check(st.inter_ts(stream, **over), "inter_residual_frame_ts")
        if "intra" in self.stages:
            check(st.intra_ts(stream, **over), "intra_recon_frame_ts")


def equal(got, want, what, chroma, skip=True):
    RC.assert_outputs_equal(got, want, what, chroma)
    if skip and "tr_skip" in want:
        np.testing.assert_array_equal(got["tr_skip"], want["tr_skip"], err_msg=what + ": tr_skip_out")


_ITEMS = {}


def items(kind):
    """the pictures of one fixture file as Items, loaded once and never changed"""
    if kind in _ITEMS:
        return _ITEMS[kind]
    out = []
    if kind == "tiles":
        z = np.load(TT.GOLDEN, allow_pickle=False)
        for pic in TC.FIXTURE_PICTURES:
            case, want = TC.load_fixture_case(z, pic)
            case.update(qp=QC.PARAMS_QP, per_lcu=True, tiled=True, lists=None, bit_cost=T.lambda_bit_cost(pic[8]))
            out.append(Item("tile_chain " + pic[0], case, ("inter", "intra"), want["full"]))
    elif kind == "plain":
        # two untiled pictures: one of lcu_qp.npz (a QP per LCU, both stages), one of intra_recon.npz (one QP, poisoned outputs, intra only)
        for p in (MC.pictures("qp")[0], MC.pictures("intra")[1], MC.pictures("qp")[2], MC.pictures("intra")[3]):
            lx, ly = QC.lcu_grid(p.w, p.h)
            col_bd, row_bd = TC.one_tile(p.w, p.h)
            case = {"name": p.name, "width": p.w, "height": p.h, "chroma": p.chroma, "signhide": p.signhide, "slice_is_intra": p.slice_is_intra,
                    "qp": p.qp, "lcu_qp": p.lcu_qp if p.lcu_qp is not None else np.full(lx * ly, p.qp, np.int8), "per_lcu": p.lcu_qp is not None,
                    "col_bd": list(col_bd), "row_bd": list(row_bd), "tiled": False, "lists": None, "bit_cost": T.lambda_bit_cost(27), "src": p.src,
                    "pred": p.pred, "cus": p.cus, "modes": p.modes}
            out.append(Item(p.name, case, p.stages, p.want, init=p.init))
    elif kind == "lists":
        z = np.load(GS.GOLDEN, allow_pickle=False)
        for pic, which in zip(SL.FIXTURE_PICTURES, ("default", "custom", "custom")):
            case = SL.load_case(z, pic)
            case.update(lists=which, bit_cost=np.array([T.lambda_bit_cost(int(q)) for q in QC.clip_qp(case["lcu_qp"]).reshape(-1)], np.int32))
            out.append(Item("scaling_list %s %s" % (pic[0], which), case, ("inter", "intra"), SL.load_want(z, pic[0], which, "full", case["chroma"]),
                            tables=SL.load_tables(z, which)))
    else:
        z, lists = np.load(TS.GOLDEN, allow_pickle=False), np.load(GS.GOLDEN, allow_pickle=False)
        for pic in T.FIXTURE_PICTURES:
            case = T.load_case(z, pic)
            tables = (lists["default_quant"], lists["default_dequant"]) if case["lists"] else None
            out.append(Item("trskip " + pic[0], case, ("inter", "intra"), T.load_want(z, pic[0], "full", case["chroma"]), tables=tables, ts=True))
    _ITEMS[kind] = out
    return out


def other_tables(it):
    """a scaling-list picture with the other set of tables, and what the fixture records for that set"""
    z = np.load(GS.GOLDEN, allow_pickle=False)
    which = "custom" if it.case["lists"] == "default" else "default"
    return it.but(case=dict(it.case, lists=which), tables=SL.load_tables(z, which), want=SL.load_want(z, it.case["name"], which, "full", it.chroma),
                  name="scaling_list %s %s" % (it.case["name"], which))


class Batch:
    """stagings and records of one call of each entry"""

    def __init__(self, A, its, init=None):
        from kvazaar_amd import _lib as B
        self.B, self.items = B, list(its)
        self.st = [it.stage(A, init[i] if init else None) for i, it in enumerate(self.items)]
        self.records = (B.ChainPictureTs * max(len(self.items), 1))(*[it.record(st) for it, st in zip(self.items, self.st)])
        self.L = B.load()

    def subset(self, stage):
        keep = [i for i, it in enumerate(self.items) if stage in it.stages]
        return (self.B.ChainPictureTs * max(len(keep), 1))(*[self.records[i] for i in keep]), len(keep)

    def run(self, stream=None):
        recs, n = self.subset("inter")
        check(self.L.kvz_hip_inter_residual_frames_ts(recs, n, stream), "inter_residual_frames_ts")
        recs, n = self.subset("intra")
        check(self.L.kvz_hip_intra_recon_frames_ts(recs, n, stream), "intra_recon_frames_ts")

    def sync(self, stream=None):
        check(self.L.kvz_hip_stream_sync(stream), "sync")

    def results(self):
        return [st.result() for st in self.st]

    def compare(self, what):
        """with each picture's fixture"""
        for it, st in zip(self.items, self.st):
            got = st.result()
            if it.want is not None:
                equal(got, it.want, "%s: %s" % (what, it.name), it.chroma, it.ts)
            if not it.ts:
                assert (got["tr_skip"] == T.POISON_SKIP).all(), "tr_skip_out was written without ts: " + it.name


def run_batch(A, its, what):
    b = Batch(A, its)
    b.run()
    b.sync()
    b.compare(what)
    return b


def groups_of(case):
    """the x extent a picture needs in the intra launches: LCU rows x tile columns"""
    return QC.lcu_grid(case["width"], case["height"])[1] * (len(case["col_bd"]) - 1)


def assert_rule(A, its, what):
    """the multi entries on one staging against the single _ts entries on a second one, both over poisoned outputs"""
    init = [it.poison() for it in its]
    b = Batch(A, its, init)
    b.run()
    b.sync()
    for i, (it, st) in enumerate(zip(its, b.st)):
        single = it.stage(A, init[i])
        it.single(single)
        single.sync()
        want, got = single.result(), st.result()
        equal(got, want, "%s: %s" % (what, it.name), it.chroma)
        if not it.cbf:
            assert (got["cbf_out"] == init[i][1]).all(), "cbf_out was written though NULL was passed"
        if not it.costs:
            np.testing.assert_array_equal(got["costs"].view(np.uint32), init[i][2].view(np.uint32), err_msg="costs were written though NULL was passed")
        if not it.ts:
            assert (got["tr_skip"] == T.POISON_SKIP).all()
        assert any((c != RC.POISON_COEFF).any() for c in got["coeff"] if c is not None), "nothing was coded"
    return b


# ---------------------------------------------------------------- 1. tiled beside untiled, flat lists
def test_tiled_pictures_beside_untiled_ones(api):
    its = items("tiles") + items("plain")[:2]
    assert [(it.case["width"], it.case["height"]) for it in its] == [(200, 136), (192, 64), (96, 72), (200, 136), (256, 192)]
    assert [it.case["tiled"] for it in its] == [True, True, True, False, False] and {it.chroma for it in its} == {0, 1}
    assert its[0].case["col_bd"] == [0, 1, 4] and its[0].case["row_bd"] == [0, 2, 3] and its[1].case["col_bd"] == [0, 1, 2, 3]
    # the grid's x extent comes from the picture with the most LCU rows x tile columns, and the others run out below it
    assert len({groups_of(it.case) for it in its}) >= 3 and max(groups_of(it.case) for it in its) == groups_of(its[0].case) == 6
    b = Batch(api, its)
    recs, n = b.subset("intra")
    assert n == 5 and [bool(recs[i].grid) for i in range(n)] == [True, True, True, False, False]
    b.run()
    b.sync()
    b.compare("tiled beside untiled")


# ---------------------------------------------------------------- 2. scaling lists
def test_scaling_list_pictures_with_default_and_custom_tables(api):
    its = items("lists")
    assert [it.case["lists"] for it in its] == ["default", "custom", "custom"] and its[1].case["tiled"] and its[1].case["per_lcu"]
    b = run_batch(api, its, "scaling lists")
    assert len({(b.records[i].tables.quant, b.records[i].tables.dequant) for i in range(3)}) == 3 and bool(b.records[1].grid)
    run_batch(api, [other_tables(it) for it in its][::-1], "scaling lists, the other set of each")


# ---------------------------------------------------------------- 3. transform skip
def test_transform_skip_with_flat_lists(api):
    its = [it for it in items("trskip") if it.tables is None]
    assert [it.case["name"] for it in its] == ["inter", "intra", "mono"]
    b = run_batch(api, its, "transform skip")
    for it, got in zip(its, b.results()):
        # the bytes of SCUs that no 4x4 luma TU covers keep their poison
        assert (got["tr_skip"] == T.POISON_SKIP).any() and (got["tr_skip"] == 1).any() and (got["tr_skip"] == 0).any(), it.name


def test_transform_skip_with_tables(api):
    mixed = [it for it in items("trskip") if it.tables is not None]
    assert len(mixed) == 1 and mixed[0].case["tiled"] and mixed[0].case["per_lcu"] and np.ndim(mixed[0].bit_cost) == 1
    its = mixed + [it.but(ts=True, bit_cost=it.case["bit_cost"], want=None) for it in items("lists")]
    assert all(np.ndim(it.bit_cost) == 1 for it in its)
    b = assert_rule(api, its, "tables and transform skip")
    np.testing.assert_array_equal(b.st[0].result()["tr_skip"], mixed[0].want["tr_skip"])
    run_batch(api, mixed + [it.but(ts=True, bit_cost=it.case["bit_cost"], want=None) for it in items("lists")[:1]], "mixed against the fixture")


# ---------------------------------------------------------------- 4. the rule itself
def rule_batches():
    tiles, plain, lists, skip = items("tiles"), items("plain"), items("lists"), items("trskip")
    flat_ts = [it for it in skip if it.tables is None]
    lcu_cost = lambda it: np.array([T.lambda_bit_cost(int(q)) for q in QC.clip_qp(it.case["lcu_qp"]).reshape(-1)], np.int32)
    return {
        "flat": [tiles[0], plain[1], tiles[1], tiles[2], plain[0]],
        "lists": [lists[0], lists[1], lists[2], other_tables(lists[0]), other_tables(lists[1])],
        "skip": [flat_ts[0], tiles[0].but(ts=True, bit_cost=lcu_cost(tiles[0]), want=None), flat_ts[1], plain[0].but(ts=True, bit_cost=31, want=None), flat_ts[2]],
        "lists and skip": [it for it in skip if it.tables is not None] + [lists[0].but(ts=True, bit_cost=lcu_cost(lists[0]), want=None),
                                                                           lists[1].but(ts=True, bit_cost=17, want=None),
                                                                           lists[2].but(ts=True, bit_cost=lcu_cost(lists[2]), want=None)],
    }


@pytest.mark.parametrize("options", ["flat", "lists", "skip", "lists and skip"])
def test_equals_the_single_picture_entries(api, options):
    """per picture the bytes kvz_hip_inter_residual_frame_ts / kvz_hip_intra_recon_frame_ts leave on a second staging, with cbf_out, costs,
    lcu_qp and lcu_bit_cost NULL for some pictures and given for others; arrays passed as NULL are not written"""
    its = rule_batches()[options]
    cbf, costs = [True, True, False, False, True], [True, False, True, False, False]
    its = [it.but(cbf=cbf[i], costs=costs[i]) for i, it in enumerate(its)]
    assert 4 <= len(its) <= 5 and {it.case["per_lcu"] for it in its} == {True, False}
    if "skip" in options:
        assert {np.ndim(it.bit_cost) for it in its} == {0, 1}
    assert_rule(api, its, options)


# ---------------------------------------------------------------- 5. sixteen pictures, order, one
def test_sixteen_pictures_order_and_one(api):
    five = items("tiles") + items("plain")[:2]
    sixteen = (five * 4)[:16]
    b = run_batch(api, sixteen, "sixteen")
    assert len(b.st) == 16 and len({st.ptr("rec", 0) for st in b.st}) == 16
    run_batch(api, five[::-1], "reversed")
    with_skip = items("trskip")[2:3] + [it.but(ts=True, bit_cost=it.case["bit_cost"], want=None) for it in items("lists")]
    fwd, rev = assert_rule(api, with_skip, "tables and transform skip"), assert_rule(api, with_skip[::-1], "tables and transform skip, reversed")
    for it, a, c in zip(with_skip, fwd.results(), rev.results()[::-1]):
        equal(a, c, "order: " + it.name, it.chroma)
    for it in five + items("trskip") + items("lists"):
        run_batch(api, [it], "alone")


# ---------------------------------------------------------------- 6. refusals
def fabricated(b, n_grids, last_grid, tail):
    """records that can only be refused: 1024 x 512 pictures (16 x 8 LCUs) on the pointers of b's first staging, moved apart so that no output is
    shared; n_grids of them with 16 x 8 tiles (26 boundaries each), one with last_grid, then `tail` ("grid": one tile as a grid, "none": no
    grid) and last a record without coeff_y, so that no such call can launch anything"""
    B = b.B
    grids = []

    def grid(cols, rows):
        g = B.TileGrid()
        g.cols, g.rows = cols, rows
        for i in range(cols + 1):
            g.col_bd[i] = i * 16 // cols
        for i in range(rows + 1):
            g.row_bd[i] = i * 8 // rows
        grids.append(g)
        return C.pointer(g)

    shapes = [(16, 8)] * n_grids + [last_grid] + [(1, 1) if tail == "grid" else None, None]
    recs = (B.ChainPictureTs * len(shapes))()
    for i, shape in enumerate(shapes):
        r = recs[i]
        C.memmove(C.byref(r), C.byref(b.records[0]), C.sizeof(r))
        r.pic.src.width, r.pic.src.height = 1024, 512
        r.pic.src.stride_y = r.pic.stride_y = 1024
        r.pic.src.stride_c = r.pic.stride_c = 512
        r.pic.rec_y, r.pic.cus, r.pic.coeff_y, r.tr_skip_out = r.pic.rec_y + 64 * i, r.pic.cus + 64 * i, r.pic.coeff_y + 64 * i, r.tr_skip_out + 64 * i
        r.grid = grid(*shape) if shape else None
    recs[len(shapes) - 1].pic.coeff_y = None
    return recs, len(shapes), grids


def test_refusals_write_nothing_and_name_the_record(api):
    from kvazaar_amd import _lib as B
    skip, lists = [it for it in items("trskip") if it.tables is None], items("lists")
    mixed = [it for it in items("trskip") if it.tables is not None] + [it.but(ts=True, bit_cost=it.case["bit_cost"], want=None) for it in lists]
    bs, bl, bm = Batch(api, skip), Batch(api, lists), Batch(api, mixed)
    L = bs.L
    before = [b.results() for b in (bs, bl, bm)]

    def bad(b, at, **fields):
        n = len(b.items)
        recs = (B.ChainPictureTs * n)(*[b.records[i] for i in range(n)])
        for k, v in fields.items():
            if k == "scaling_list":
                recs[at].pic.params.scaling_list = v
            elif k == "tables":
                recs[at].tables = v
            else:
                setattr(recs[at], k, v)
        return recs, n, at

    some = bl.records[0].tables
    none = B.ScalingTables(None, None)
    half = B.ScalingTables(some.quant, None)
    w, h = mixed[0].case["width"], mixed[0].case["height"]
    short = api.tile_grid(w, h, [0, 1, 2], mixed[0].case["row_bd"])          # the last boundary is 2 of 3 LCUs
    short_p = C.cast(short.ctypes.data, C.POINTER(B.TileGrid))
    both = [
        bad(bs, 2, tables=some, scaling_list=1),                 # a record with tables among records without
        bad(bl, 1, tables=none, scaling_list=0),                 # and one without among records with
        bad(bl, 2, ts=bs.records[0].ts, tr_skip_out=bs.records[0].tr_skip_out),   # a record with ts among records without
        bad(bm, 1, ts=None),                                     # and one without among records with
        bad(bs, 1, scaling_list=1),                              # scaling_list set without tables
        bad(bl, 1, scaling_list=0),                              # tables without scaling_list
        bad(bl, 2, tables=half),                                 # a NULL table
        bad(bs, 1, tr_skip_out=None),                            # ts without tr_skip_out
        bad(bm, 3, tr_skip_out=bm.records[1].tr_skip_out),       # a shared tr_skip_out
    ]
    intra_only = [bad(bm, 0, grid=short_p)]                      # the inter stage does not depend on tiles and does not read the grid
    for entry in (L.kvz_hip_inter_residual_frames_ts, L.kvz_hip_intra_recon_frames_ts):
        for recs, n, at in both + (intra_only if entry is L.kvz_hip_intra_recon_frames_ts else []):
            assert entry(recs, n, None) == INVALID, at
            assert b"picture %d (" % at in L.kvz_hip_last_error(), (at, L.kvz_hip_last_error())
        assert entry(bs.records, 0, None) == 0 and entry(None, 0, None) == 0
        assert entry(bs.records, 17, None) == INVALID and entry(bs.records, -1, None) == INVALID and entry(None, 3, None) == INVALID
    # the pool of boundaries: 9 x 26 + 22 = 256 fit, and the call goes on to refuse its last record; 9 x 26 + 19 + 4 = 257 do not, and the
    # record that overflowed is named
    assert B.CHAIN_TILE_BOUNDS == 256
    recs, n, keep = fabricated(bs, 9, (12, 8), "none")
    assert L.kvz_hip_intra_recon_frames_ts(recs, n, None) == INVALID and b"picture 11 (" in L.kvz_hip_last_error(), L.kvz_hip_last_error()
    recs, n, keep = fabricated(bs, 9, (9, 8), "grid")
    assert L.kvz_hip_intra_recon_frames_ts(recs, n, None) == INVALID and b"picture 10 (" in L.kvz_hip_last_error(), L.kvz_hip_last_error()
    assert b"KVZ_HIP_CHAIN_TILE_BOUNDS" in L.kvz_hip_last_error()
    bs.sync()
    for b, was in zip((bs, bl, bm), before):
        for it, got, want in zip(b.items, b.results(), was):
            equal(got, want, it.name + " after refused calls", it.chroma)
            assert (got["tr_skip"] == T.POISON_SKIP).all()
    assert L.kvz_hip_abi_version() == 4
    # and the same records are accepted as they stand
    for b in (bs, bl):
        b.run()
        b.sync()
        b.compare("after the refusals")


# ---------------------------------------------------------------- 7. no options
def test_without_options_it_is_the_plain_multi_picture_entries(api):
    its = items("plain")
    new, old = Batch(api, its), Batch(api, its)
    new.run()
    new.sync()
    B, L = old.B, old.L
    for stage, entry in (("inter", L.kvz_hip_inter_residual_frames), ("intra", L.kvz_hip_intra_recon_frames)):
        recs, n = old.subset(stage)
        assert not any(bool(recs[i].grid) or recs[i].tables.quant or bool(recs[i].ts) for i in range(n))
        plain = (B.ChainPicture * n)(*[recs[i].pic for i in range(n)])
        check(entry(plain, n, None), "the plain multi-picture entry")
    old.sync()
    for it, a, c in zip(its, new.results(), old.results()):
        equal(a, c, "no options: " + it.name, it.chroma)
        equal(a, it.want, "no options, fixture: " + it.name, it.chroma)


# ---------------------------------------------------------------- 8. graph
def test_both_calls_replayed_from_a_graph_after_the_contents_changed(api):
    """a tiled batch with transform skip, captured on one stream; the replay runs on other sources and bit costs in two of the three
    pictures and equals the single entries run on those"""
    tiles, skip = items("tiles"), items("trskip")
    cost = lambda it, k: np.array([T.lambda_bit_cost(int(q)) + k for q in QC.clip_qp(it.case["lcu_qp"]).reshape(-1)], np.int32)
    its = [tiles[0].but(ts=True, bit_cost=cost(tiles[0], 0), want=None), skip[1], tiles[2].but(ts=True, bit_cost=cost(tiles[2], 0), want=None)]
    b = Batch(api, its)
    L, s, graph = b.L, b.L.kvz_hip_stream_create(), C.c_void_p()
    try:
        check(L.kvz_hip_graph_begin(s), "graph_begin")
        b.run(s)
        check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        changed = [its[0].but(case=dict(its[0].case, src=tuple(np.ascontiguousarray(p[::-1, ::-1]) for p in its[0].case["src"])), bit_cost=cost(its[0], 9)),
                   its[1],
                   its[2].but(case=dict(its[2].case, src=(np.ascontiguousarray(its[2].case["src"][0][::-1]), None, None)), bit_cost=cost(its[2], 40))]
        wants = {}
        for run, now in (("first launch", its), ("replay", changed)):
            want = wants[run] = []
            for it, st in zip(now, b.st):
                single = it.stage(api)
                it.single(single)
                single.sync()
                want.append(single.result())
                for k in range(3 if it.chroma else 1):
                    st.upload("src", k, it.case["src"][k], s)
                st.host["src"] = [np.ascontiguousarray(p) for p in it.case["src"][:3 if it.chroma else 1]]
                if np.ndim(it.bit_cost):
                    st.upload("bit_cost", 0, np.asarray(it.bit_cost, np.int32), s)
                    st.host["bit_cost"] = [np.asarray(it.bit_cost, np.int32)]
                for kind in ("rec", "coeff", "cus", "cbf_out", "costs", "tr_skip"):
                    for k, a in enumerate(st.host[kind]):
                        st.upload(kind, k, a, s)
            b.sync(s)
            check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            b.sync(s)
            for it, st, w in zip(now, b.st, want):
                equal(st.result(), w, "%s: %s" % (run, it.name), it.chroma)
        for i in (0, 2):
            assert not np.array_equal(wants["replay"][i]["rec"][0], wants["first launch"][i]["rec"][0]), "the replay ran on other contents"
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


# ---------------------------------------------------------------- 9. numpy conveniences
def test_numpy_conveniences_on_a_tiled_and_a_transform_skip_batch(api):
    def plain(it):
        c, init = it.case, QC.zero_outputs(it.case["width"], it.case["height"], it.chroma)
        return dict(src=c["src"], pred=c["pred"], cus=c["cus"], qp=c["qp"], chroma=it.chroma, slice_is_intra=c["slice_is_intra"], signhide=c["signhide"],
                    coeff=init[0], cbf_out=init[1], costs=init[2], lcu_qp=c["lcu_qp"] if c["per_lcu"] else None)

    def second(it, d, m, **more):
        return dict(d, src=it.case["src"], rec=m["rec"], cus=m["cus"], modes=it.case["modes"], coeff=m["coeff"], cbf_out=m["cbf_out"], costs=m["costs"], **more)

    tiles = items("tiles")
    first = [plain(it) for it in tiles]
    mid = api.inter_residual_frames_ts(first)
    for d in first:
        del d["pred"]
    full = api.intra_recon_frames_ts([second(it, d, m, grid=(it.case["col_bd"], it.case["row_bd"])) for it, d, m in zip(tiles, first, mid)])
    for it, got in zip(tiles, full):
        RC.assert_outputs_equal(got, it.want, it.name + " convenience", it.chroma)
        assert "tr_skip_out" not in got
    skip = [it for it in items("trskip") if it.tables is None]
    poison = lambda it: np.full(it.case["cus"].shape, T.POISON_SKIP, np.uint8)
    first = [dict(plain(it), trskip=dict(bit_cost=int(it.bit_cost)), tr_skip_out=poison(it)) for it in skip]
    mid = api.inter_residual_frames_ts(first)
    for d in first:
        del d["pred"], d["tr_skip_out"]
    full = api.intra_recon_frames_ts([second(it, d, m, tr_skip_out=m["tr_skip_out"]) for it, d, m in zip(skip, first, mid)])
    for it, got in zip(skip, full):
        RC.assert_outputs_equal(got, it.want, it.name + " convenience", it.chroma)
        np.testing.assert_array_equal(got["tr_skip_out"], it.want["tr_skip"])
    assert api.inter_residual_frames_ts([]) == [] and api.intra_recon_frames_ts([]) == []
